"""Writes tests/golden/matcher_expected.npz (build container only) by running the REFERENCE's own Matching module (SuperPoint, then SuperGlue) and
SuperPoint's helper functions (estimate_pose/glue_match.py, superpoint.py, superglue.py) on the seeded inputs of matcher_cases.py, in eval() on the CPU, float32.

The modules' constructors call torch.load on weight files the tree does not contain; for those loads, inside this process only, the
seeded state dicts of matcher_cases.superpoint_state / superglue_state are handed over instead.  Only inputs and results are stored: the weights come from
the seed.  The logits and raw descriptors are what the module's own convPb / convDb return, mdesc what final_proj returns (forward hooks).
Every case must have a match, an unmatched keypoint, and at most one keypoint in eight undecided between float32 and float64.
Run:  python tests/golden/make_matcher_golden.py"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import matcher_cases as C  # noqa: E402
import matcher_reference as R  # noqa: E402
import parity_rule as PR  # noqa: E402
import ref_import  # noqa: E402


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)                                               # one summation order, whatever the host
    sys.path.insert(0, ref_import.REFERENCE_ROOT)
    try:
        sp = importlib.import_module("estimate_pose.superpoint")
        gm = importlib.import_module("estimate_pose.glue_match")
    finally:
        sys.path.remove(ref_import.REFERENCE_ROOT)
    state, glue = C.superpoint_state(), C.superglue_state()
    real_load = torch.load
    out = {}
    for name, (H, W, _, radius, thr, maxk, border) in C.PAIRS.items():
        torch.load = lambda path, *a, **k: state if "superpoint" in str(path) else glue
        try:
            net = gm.Matching({"superpoint": dict(nms_radius=radius, keypoint_threshold=thr, max_keypoints=maxk, remove_borders=border),
                               "superglue": dict(GNN_layers=list(C.GNN_LAYERS), sinkhorn_iterations=C.SINKHORN_ITERATIONS,
                                                 match_threshold=C.MATCH_THRESHOLD)}).eval()
        finally:
            torch.load = real_load
        seen = {"logits": [], "raw": [], "mdesc": []}
        net.superpoint.convPb.register_forward_hook(lambda m, i, o: seen["logits"].append(o.detach().clone()))
        net.superpoint.convDb.register_forward_hook(lambda m, i, o: seen["raw"].append(o.detach().clone()))
        net.superglue.final_proj.register_forward_hook(lambda m, i, o: seen["mdesc"].append(o.detach().clone()))
        im = C.pair_images(name)
        with torch.no_grad():
            got = net({"image0": torch.from_numpy(im[0])[None, None], "image1": torch.from_numpy(im[1])[None, None]})
        out[f"{name}.image"] = im
        out[f"{name}.logits"] = torch.cat(seen["logits"]).permute(0, 2, 3, 1).contiguous().numpy()
        out[f"{name}.raw"] = torch.cat(seen["raw"]).permute(0, 2, 3, 1).contiguous().numpy()
        for i in range(2):
            out[f"{name}.kpts{i}"] = got[f"keypoints{i}"][0].numpy()
            out[f"{name}.scores{i}"] = got[f"scores{i}"][0].numpy()
            out[f"{name}.desc{i}"] = got[f"descriptors{i}"][0].t().contiguous().numpy()          # [N, 256]
            out[f"{name}.mdesc{i}"] = seen["mdesc"][i][0].t()[:C.MDESC_PROBE].contiguous().numpy()  # the first rows: a probe, the rest follows from the matches
            out[f"{name}.matches{i}"] = got[f"matches{i}"][0].numpy()
            out[f"{name}.matching_scores{i}"] = got[f"matching_scores{i}"][0].numpy()
        counts = [len(got[f"keypoints{i}"][0]) for i in range(2)]
        m0 = got["matches0"][0]
        print(name, "keypoints", counts, "matches", int((m0 > -1).sum()))
        assert min(counts) >= 8
        if name == "topk":
            assert counts == [maxk, maxk]
        else:
            assert max(counts) < maxk
        if name == "unequal":
            assert counts[0] != counts[1]
        assert int((m0 > -1).sum()) >= 1, "every case has a match"
        assert int((m0 == -1).sum()) >= 1, "every case has an unmatched keypoint"
        # the decided-share cap of the GPU suite, for the reference alone: float32 against the float64 restatement
        shape, z = (H, W), {}
        for dt in (torch.float32, torch.float64):
            res, _ = R.superpoint(state, torch.from_numpy(im), radius, thr, maxk, border, dtype=dt)
            (a, _), (b, _) = R.match_descriptors(glue, C.GNN_LAYERS, res[0]["keypoints"], res[0]["scores"], res[0]["descriptors"], shape,
                                                 res[1]["keypoints"], res[1]["scores"], res[1]["descriptors"], shape, dt)
            z[dt] = R.transport(a, b, C.BIN_SCORE, C.SINKHORN_ITERATIONS, dt)
        (z32, _), (z64, bound) = z[torch.float32], z[torch.float64]
        tol = PR.tolerance(PR.ratio(z32, z64, bound)) * bound
        d0, d1 = R.decided(z64, tol)
        undecided = int((~d0).sum()) + int((~d1).sum())
        print("  undecided", undecided, "of", len(d0) + len(d1))
        assert undecided * 8 <= len(d0) + len(d1), "at most one keypoint in eight may be undecided"
    maps = C.crafted_maps()
    for key, m in maps.items():
        out[f"map.{key}"] = m
        for r in C.NMS_RADII:
            out[f"nms.{key}.r{r}"] = sp.simple_nms(torch.from_numpy(m)[None], r)[0].numpy()
    for k, (key, r, thr, border, maxk) in enumerate(C.SELECTIONS):
        kept = sp.simple_nms(torch.from_numpy(maps[key])[None], r)[0]
        kp = torch.nonzero(kept > thr)
        sc = kept[tuple(kp.t())]
        kp, sc = sp.remove_borders(kp, sc, border, *kept.shape)
        if len(sc) > maxk:
            assert len(torch.unique(sc)) == len(sc), "equal scores at a cut: the reference leaves the choice to torch.topk"
        kp, sc = sp.top_k_keypoints(kp, sc, maxk)
        out[f"sel.{k}.kpts"] = torch.flip(kp, [1]).float().numpy()
        out[f"sel.{k}.scores"] = sc.numpy()
        print("selection", k, key, "->", len(sc))
    np.savez_compressed(os.path.join(HERE, "matcher_expected.npz"), **out)
    print("wrote", len(out), "arrays,", os.path.getsize(os.path.join(HERE, "matcher_expected.npz")), "bytes")


if __name__ == "__main__":
    main()
