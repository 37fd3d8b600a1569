"""CPU checks of the SuperPoint and SuperGlue restatement (tests/matcher_reference.py) against the reference's own float32 outputs in
tests/golden/matcher_expected.npz, of the BatchNorm fold and head permutation as algebra, of the unposed script's pose sources, and of
everything SuperPoint's entries refuse without launching.

The arithmetic stages are held to the fixture by parity_rule: the fixture's distance to the float64 restatement over the bound may be
8 x the float32 restatement's own (both are float32 runs of one formula; they differ in summation order at most).  The decision stages
(suppression, selection) only compare, so they are held to the reference's functions bit for bit."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import matcher_cases as C  # noqa: E402
import matcher_reference as R  # noqa: E402
import parity_rule as PR  # noqa: E402

F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module", autouse=True)
def one_thread():
    """The generator ran torch on one thread; the float32 restatement's sums take the same order here, whatever the host's core count."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.fixture(scope="module")
def golden():
    return {k: torch.from_numpy(v) for k, v in np.load(os.path.join(HERE, "golden", "matcher_expected.npz")).items()}


@pytest.fixture(scope="module")
def state():
    return C.superpoint_state()


@pytest.fixture(scope="module")
def runs(golden, state):
    """Both precisions of every pair, computed once."""
    out = {}
    for name, (_, _, _, radius, thr, maxk, border) in C.PAIRS.items():
        im = golden[f"{name}.image"]
        out[name] = {dt: R.superpoint(state, im, radius, thr, maxk, border, dtype=dt) for dt in (F32, F64)}
    return out


def test_the_images_come_from_the_seed(golden):
    for name in C.PAIRS:
        assert np.array_equal(golden[f"{name}.image"].numpy(), C.pair_images(name))
    for key, m in C.crafted_maps().items():
        assert np.array_equal(golden[f"map.{key}"].numpy(), m)


@pytest.mark.parametrize("name", sorted(C.PAIRS))
def test_restatement_reproduces_the_reference(golden, runs, name):
    (res32, d32), (res64, d64) = runs[name][F32], runs[name][F64]
    entries = {}
    for what in ("logits", "raw"):
        bound = d64["bound_" + what]
        entries[what] = ((golden[f"{name}.{what}"], d64[what], bound), PR.ratio(d32[what], d64[what], bound))
    PR.judge("matcher_reference", f"{name} dense", entries)
    for i in range(2):
        assert torch.equal(res32[i]["keypoints"], golden[f"{name}.kpts{i}"]), "keypoint set or order"
        assert torch.equal(res64[i]["keypoints"], golden[f"{name}.kpts{i}"]), "the float64 restatement decides differently"
        pix = golden[f"{name}.kpts{i}"].long()
        bs = d64["bound_scores"][i][pix[:, 1], pix[:, 0]]
        PR.judge("matcher_reference", f"{name} image {i}", {
            "scores": ((golden[f"{name}.scores{i}"], res64[i]["scores"], bs), PR.ratio(res32[i]["scores"], res64[i]["scores"], bs)),
            "descriptors": ((golden[f"{name}.desc{i}"], res64[i]["descriptors"], res64[i]["bound_descriptors"]),
                            PR.ratio(res32[i]["descriptors"], res64[i]["descriptors"], res64[i]["bound_descriptors"]))})
    maxk = C.PAIRS[name][5]
    counts = [len(res32[i]["keypoints"]) for i in range(2)]
    if name == "topk":
        assert counts == [maxk, maxk]
        for i in range(2):
            s = res32[i]["scores"]
            assert bool((s[:-1] >= s[1:]).all()), "the top-k's order is descending score"
    else:
        for i in range(2):
            k = res32[i]["keypoints"]
            idx = k[:, 1] * 1e4 + k[:, 0]
            assert bool((idx[:-1] < idx[1:]).all()), "nothing cut: row-major order"


def test_nms_restated_is_the_reference_bit_for_bit(golden):
    for key in C.crafted_maps():
        for r in C.NMS_RADII:
            got = R.nms(golden[f"map.{key}"], r)
            assert torch.equal(got.view(torch.int32), golden[f"nms.{key}.r{r}"].view(torch.int32)), (key, r)


def test_selection_restated_is_the_reference_bit_for_bit(golden):
    for k, (key, r, thr, border, maxk) in enumerate(C.SELECTIONS):
        kp, sc = R.select(R.nms(golden[f"map.{key}"], r), thr, border, maxk)
        assert torch.equal(kp, golden[f"sel.{k}.kpts"].reshape(-1, 2)), (k, key)
        assert torch.equal(sc.view(torch.int32), golden[f"sel.{k}.scores"].view(torch.int32)), (k, key)
    empty = [k for k, s in enumerate(C.SELECTIONS) if golden[f"sel.{k}.scores"].numel() == 0]
    assert len(empty) >= 3                      # everything under the threshold, everything inside the border, a border that leaves nothing


def test_equal_scores_go_to_the_lower_row_major_index():
    m = torch.zeros(8, 8)
    m[1, 5] = m[2, 2] = m[6, 1] = 0.5
    m[4, 4] = 0.75
    kp, sc = R.select(m, 0.1, 0, 3)
    assert kp.tolist() == [[4.0, 4.0], [5.0, 1.0], [2.0, 2.0]] and sc.tolist() == [0.75, 0.5, 0.5]
    kp, _ = R.select(m, 0.1, 0, 4)
    assert kp.tolist() == [[5.0, 1.0], [2.0, 2.0], [4.0, 4.0], [1.0, 6.0]]


# ---- the host interface and the entries' refusals: nothing here launches, so no device is needed ----
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from cross_attention_renderer_amd import _lib
    return _lib.load()


def test_weights_are_validated_by_name(state):
    from cross_attention_renderer_amd import matching as M
    assert M.SUPERPOINT_CONVS == C.SUPERPOINT_CONVS
    w = M.MatcherWeights(state)
    assert len(w.conv_w) == 12 and w.conv_w[9].shape == (65, 256, 1, 1)
    with pytest.raises(ValueError, match="'convPb.bias' is missing"):
        M.MatcherWeights({k: v for k, v in state.items() if k != "convPb.bias"})
    with pytest.raises(ValueError, match=r"'conv3a.weight' has shape \(128, 64, 1, 1\)"):
        M.MatcherWeights(dict(state, **{"conv3a.weight": state["conv3a.weight"][:, :, :1, :1]}))
    with pytest.raises(ValueError, match="no CPU fallback"):
        w.packed("cpu")


def test_superpoint_refuses_cpu_tensors_and_bad_arguments(state):
    from cross_attention_renderer_amd import matching as M
    w = M.MatcherWeights(state)
    with pytest.raises(ValueError, match="no CPU fallback"):
        M.superpoint(torch.zeros(16, 16), w)
    with pytest.raises(ValueError, match="must be a tensor"):
        M.superpoint(np.zeros((16, 16), np.float32), w)


def test_entries_refuse_without_launching(lib):
    one = ctypes.c_void_p(16)                                            # a non-null, aligned address that nothing may touch
    err = lambda: lib.car_last_error().decode()
    # conv1a's 9 x 64 weights and bias; nine 3 x 3 layers as 9 K / 32 x N / 16 tiles of 512 floats, 64 floats of scale and the bias; the two heads
    conv = lambda K, N: 9 * K // 32 * (N // 16) * 512 + 64 + N
    assert lib.car_superpoint_packed_floats() == (640 + 3 * conv(64, 64) + conv(64, 128) + 3 * conv(128, 128) + 2 * conv(128, 256)
                                                  + lib.car_linear_packed_floats(256, 65) + lib.car_linear_packed_floats(256, 256))
    for h, w in ((12, 16), (16, 20), (0, 8), (8, 4)):
        assert lib.car_superpoint_workspace_bytes(1, h, w) == 0 and "multiples of 8" in err()
        assert lib.car_superpoint_dense(one, 1, h, w, one, one, one, one, 1 << 30, None) == -1 and "multiples of 8" in err()
    assert lib.car_superpoint_workspace_bytes(2, 256, 256) == 2 * 2 * 256 * 256 * 64 * 4
    assert lib.car_superpoint_workspace_bytes(1, 4096, 4096) == 0
    assert lib.car_superpoint_dense(one, 1, 16, 16, one, one, one, one, lib.car_superpoint_workspace_bytes(1, 16, 16) - 1, None) == -1 and "workspace holds" in err()
    assert lib.car_superpoint_dense(None, 1, 16, 16, one, one, one, one, 1 << 30, None) == -1 and "null pointer" in err()
    assert lib.car_superpoint_pack(None, None, None, None) == -1 and "null pointer" in err()
    table = (ctypes.c_void_p * 12)(*([16] * 11 + [None]))
    assert lib.car_superpoint_pack(table, table, one, None) == -1 and "convolution 11" in err()
    assert lib.car_superpoint_conv1a(one, 1, 0, 8, one, one, None) == -1
    assert lib.car_superpoint_conv1a(None, 1, 8, 8, one, one, None) == -1 and "null pointer" in err()
    for r in (-1, 9):
        assert lib.car_superpoint_nms(one, 1, 8, 8, r, ctypes.c_void_p(32), one, 1 << 20, None) == -1 and "need 0..8" in err()
    assert lib.car_superpoint_nms(one, 1, 8, 8, 4, one, one, 1 << 20, None) == -1 and "must not be the score map" in err()
    assert lib.car_superpoint_nms(one, 1, 8, 8, 4, ctypes.c_void_p(32), one, 3 * 64 * 4 - 1, None) == -1 and "workspace holds" in err()
    assert lib.car_superpoint_nms(one, 1, 8, 8, 4, None, one, 1 << 20, None) == -1 and "null pointer" in err()
    assert lib.car_superpoint_nms_workspace_bytes(1, 8, 8) == 3 * 64 * 4 and lib.car_superpoint_select_workspace_bytes(2, 8, 16) == 2 * 128 * 4
    for maxk, text in ((0, "need 1..4096"), (4097, "need 1..4096"), (-1, "is not served"), (-2, "need 1..4096")):
        assert lib.car_superpoint_select(one, 1, 8, 8, 0.005, 4, maxk, one, one, one, one, 1 << 20, None) == -1 and text in err(), maxk
    assert lib.car_superpoint_select(one, 1, 8, 8, float("nan"), 4, 10, one, one, one, one, 1 << 20, None) == -1 and "NaN" in err()
    assert lib.car_superpoint_select(one, 1, 8, 8, 0.005, -1, 10, one, one, one, one, 1 << 20, None) == -1 and "border" in err()
    assert lib.car_superpoint_select(one, 1, 8, 8, 0.005, 4, 10, one, one, one, one, 255, None) == -1 and "workspace holds" in err()
    assert lib.car_superpoint_select(one, 1, 8, 8, 0.005, 4, 10, one, one, None, one, 256, None) == -1 and "null pointer" in err()
    for n in (0, 4097):
        assert lib.car_superpoint_sample(one, n, one, 1, 1, one, None) == -1 and "need 1..4096" in err()
    assert lib.car_superpoint_sample(one, 5, one, 0, 1, one, None) == -1
    assert lib.car_superpoint_sample(one, 5, ctypes.c_void_p(20), 1, 1, one, None) == -1 and "16-byte aligned" in err()
    assert lib.car_superpoint_sample(one, 5, None, 1, 1, one, None) == -1 and "null pointer" in err()


# ---- SuperGlue --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def glue():
    return C.superglue_state()


@pytest.mark.parametrize("name", sorted(C.PAIRS))
def test_superglue_restatement_reproduces_the_reference(golden, glue, runs, name):
    """mdesc (the fixture's probe rows) and the matching scores by the yardstick rule, the matches exactly; both from the float32
    restatement, which runs the reference's own sequence of torch operations."""
    H, W = C.PAIRS[name][:2]
    out = {}
    for dt in (F32, F64):
        res = runs[name][dt][0]
        md = R.match_descriptors(glue, C.GNN_LAYERS, res[0]["keypoints"], res[0]["scores"], res[0]["descriptors"], (H, W), res[1]["keypoints"],
                                 res[1]["scores"], res[1]["descriptors"], (H, W), dt)
        Z, bound = R.transport(md[0][0], md[1][0], C.BIN_SCORE, C.SINKHORN_ITERATIONS, dt)
        out[dt] = (md, Z, bound, R.matches(Z, C.MATCH_THRESHOLD))
    (md32, z32, _, w32), (md64, z64, bound, w64) = out[F32], out[F64]
    n = C.MDESC_PROBE
    PR.judge("matcher_reference", f"{name} mdesc", {f"mdesc{i}": ((golden[f"{name}.mdesc{i}"], md64[i][0][:n], md64[i][1][:n]),
                                                                  PR.ratio(md32[i][0][:n], md64[i][0][:n], md64[i][1][:n])) for i in range(2)})
    d = R.decided(z64, PR.tolerance(PR.ratio(z32, z64, bound)) * bound)
    entries = {}
    for i in range(2):
        assert torch.equal(w32[i], golden[f"{name}.matches{i}"].long()), (name, i, "matches")
        assert torch.equal(w32[i][d[i]], w64[i][d[i]]), (name, i, "a decided match differs between the precisions")
        zi, bi = (z64[:-1, :-1], bound[:-1, :-1]) if i == 0 else (z64[:-1, :-1].t(), bound[:-1, :-1].t())
        at = zi.argmax(1)
        sb = w64[2 + i].double() * bi[torch.arange(len(at)), at]                       # |d exp(Z)| = exp(Z) |dZ|
        entries[f"scores{i}"] = ((golden[f"{name}.matching_scores{i}"], w64[2 + i], sb, d[i]), PR.ratio(w32[2 + i], w64[2 + i], sb, d[i]))
    PR.judge("matcher_reference", f"{name} matching scores where decided", entries)
    assert int((w32[0] > -1).sum()) >= 1 and int((w32[0] == -1).sum()) >= 1
    assert 8 * sum(int((~x).sum()) for x in d) <= sum(len(x) for x in d), "at most one keypoint in eight undecided"

def test_fold_and_head_permutation_are_algebra(golden, glue, runs):
    """The BatchNorm fold and the head permutation change nothing: the folded, head-contiguous network against the plain one in float64,
    to 1e-12 of the summed magnitudes."""
    fold = R.folded(glue, len(C.GNN_LAYERS))
    assert not any("running" in k for k in fold)
    for name in ("topk", "unequal"):
        H, W = C.PAIRS[name][:2]
        res = runs[name][F64][0]
        args = (res[0]["keypoints"], res[0]["scores"], res[0]["descriptors"], (H, W), res[1]["keypoints"], res[1]["scores"], res[1]["descriptors"], (H, W))
        plain = R.match_descriptors(glue, C.GNN_LAYERS, *args, F64)
        got = R.match_descriptors_folded(fold, C.GNN_LAYERS, *args)
        for i in range(2):
            assert PR.ratio(got[i], plain[i][0], plain[i][1]) <= 1e-12, (name, i)
    # a contiguous block per head instead of the stride-4 split gives plausible but different numbers: the check must see it
    wrong = dict(fold)
    for l in range(len(C.GNN_LAYERS)):
        for j in range(3):
            wrong[f"gnn.layers.{l}.attn.proj.{j}.weight"] = glue[f"gnn.layers.{l}.attn.proj.{j}.weight"].double()
            wrong[f"gnn.layers.{l}.attn.proj.{j}.bias"] = glue[f"gnn.layers.{l}.attn.proj.{j}.bias"].double()
        wrong[f"gnn.layers.{l}.attn.merge.weight"] = glue[f"gnn.layers.{l}.attn.merge.weight"].double()
    bad = R.match_descriptors_folded(wrong, C.GNN_LAYERS, *args)
    assert PR.ratio(bad[0], plain[0][0], plain[0][1]) > 1e-4


def test_match_rule_on_crafted_scores():
    Z = torch.tensor([[0.0, -1.0, -9.0], [-1.0, -0.5, -9.0], [-1.0, -3.0, -9.0], [-9.0, -9.0, -9.0]])     # 3 x 2 and the dustbin
    m0, m1, s0, s1 = R.matches(Z, 0.2)
    assert m0.tolist() == [0, 1, -1] and m1.tolist() == [0, 1]
    assert torch.allclose(s0, torch.tensor([1.0, 0.6065307, 0.0])) and torch.allclose(s1, torch.tensor([1.0, 0.6065307]))
    m0, m1, _, _ = R.matches(Z, 0.7)                                       # the threshold removes the weaker mutual pair on both sides
    assert m0.tolist() == [0, -1, -1] and m1.tolist() == [0, -1]
    m0, m1, s0, _ = R.matches(torch.zeros(3, 4), 0.2)                      # all tied: every arg-max is index 0, one mutual pair
    assert m0.tolist() == [0, -1] and m1.tolist() == [0, -1, -1] and s0.tolist() == [1.0, 0.0]
    assert [d.tolist() for d in R.decided(Z.double(), 0.1)] == [[True, True, True], [True, True]]
    d0, d1 = R.decided(Z.double(), 0.3)                                    # row 1 and column 1 lead by 0.5 only: not twice the tolerance
    assert d0.tolist() == [True, False, True] and d1.tolist() == [True, False]


def test_superglue_weights_are_validated_by_name(state, glue):
    from cross_attention_renderer_amd import matching as M
    w = M.MatcherWeights(state, glue)
    assert w.gnn_layers == list(C.GNN_LAYERS) and len(w.glue) == 26 + 16 * 4 + 2 and abs(w.bin_score - C.BIN_SCORE) < 1e-6
    with pytest.raises(ValueError, match=r"'gnn.layers.2.mlp.1.running_var' is missing"):
        M.MatcherWeights(state, {k: v for k, v in glue.items() if k != "gnn.layers.2.mlp.1.running_var"})
    with pytest.raises(ValueError, match=r"'kenc.encoder.0.weight' has shape \(32, 2, 1\)"):
        M.MatcherWeights(state, dict(glue, **{"kenc.encoder.0.weight": glue["kenc.encoder.0.weight"][:, :2]}))
    with pytest.raises(ValueError, match="zero GNN layers"):
        M.MatcherWeights(state, {k: v for k, v in glue.items() if not k.startswith("gnn.")})
    with pytest.raises(ValueError, match="'self' or 'cross'"):
        M.MatcherWeights(state, glue, ["self", "both"])
    with pytest.raises(ValueError, match="no CPU fallback"):
        w.packed_glue("cpu")
    with pytest.raises(ValueError, match="no CPU fallback"):
        z = torch.zeros(3, 2), torch.zeros(3), torch.zeros(3, 256)
        M.superglue(*z, *z, (16, 16), w)


def test_the_three_pose_sources_are_mutually_exclusive():
    import argparse
    import importlib.util
    spec = importlib.util.spec_from_file_location("render_unposed_traj", os.path.join(os.path.dirname(HERE), "experiment_scripts", "render_unposed_traj.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    base = dict(im1="a.npy", im2="b.npy", synthetic=False, matches=None, pose=None, matcher_weights=None, save_matches=None)
    opt = lambda **kw: argparse.Namespace(**dict(base, **kw))
    for one in (dict(matches="m.npz"), dict(pose="p.npz"), dict(matcher_weights=["a.pth", "b.pth"]), dict(matcher_weights=["a.pth", "b.pth"], save_matches="o.npz")):
        script.check_pose_sources(opt(**one))
    with pytest.raises(SystemExit, match="exactly one of --matches \\(SuperGlue's .npz for the pair\\) and --pose"):
        script.check_pose_sources(opt())
    with pytest.raises(SystemExit, match="exactly one of --matches \\(SuperGlue's .npz for the pair\\) and --pose"):
        script.check_pose_sources(opt(matches="m.npz", pose="p.npz"))
    for two in (dict(matches="m.npz", matcher_weights=["a", "b"]), dict(pose="p.npz", matcher_weights=["a", "b"]),
                dict(synthetic=True, matches="m.npz", matcher_weights=["a", "b"]), dict(synthetic=True, matches="m.npz", pose="p.npz")):
        with pytest.raises(SystemExit, match="both name the relative pose"):
            script.check_pose_sources(opt(**two))
    with pytest.raises(SystemExit, match="needs --matcher_weights"):
        script.check_pose_sources(opt(matches="m.npz", save_matches="o.npz"))
    script.check_pose_sources(opt(synthetic=True))                         # the synthetic pair with its own pose: as before
    g = script.gray(np.array([[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], [[0.0, 0.0, 1.0], [1.0, 1.0, 1.0]]]))
    assert np.allclose(g, [[0.2125, 0.7154], [0.0721, 1.0]], atol=1e-15)


def test_match_signatures_mirror_their_header_type_by_type(lib):
    """include/car_match.h against _lib.MATCH_SIGNATURES, by test_abi's own comparison: names, return types, arity, each parameter's kind.
    The header is included by car_hip.h and holds nothing but the matcher's entries; every one is exported and bound on both handles."""
    import re
    import test_abi as T
    from cross_attention_renderer_amd import _lib
    root = os.path.dirname(HERE)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "car_match.h")).read(), flags=re.S)
    text = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("#"))
    protos = {}
    for ret, name, params in re.findall(r"([\w \*]+?)\s*\b(car_\w+)\s*\(([^)]*)\)\s*;", text):
        params = [p.strip() for p in " ".join(params.split()).split(",")]
        params = [] if params == ["void"] else ["*" if "*" in p else " ".join(w for w in p.split()[:-1] if w != "const") for p in params]
        protos[name] = (" ".join(ret.split()).replace(" *", "*"), params)
    assert len(protos) == 19 == len(_lib.MATCH_SIGNATURES) and not set(protos) & set(_lib.SIGNATURES)
    assert T._abi_disagreements(protos, _lib.MATCH_SIGNATURES) == []
    assert all(n.startswith(("car_superpoint_", "car_superglue_")) for n in protos)
    assert '#include "car_match.h"' in open(os.path.join(root, "include", "car_hip.h")).read()
    api = _lib.api()
    for name, (res, _) in _lib.MATCH_SIGNATURES.items():
        assert hasattr(lib, name), name
        assert (getattr(api, name).errcheck is _lib._errcheck) == (res is ctypes.c_int), name          # no value entries among them
        assert getattr(lib, name).errcheck is not _lib._errcheck, name
    with pytest.raises(_lib.CarError, match="null pointer"):
        api.car_superpoint_pack(None, None, None, None)
