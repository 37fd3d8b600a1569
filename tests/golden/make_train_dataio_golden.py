"""Writes the training-reader fixture (build container only): what the REFERENCE's ``RealEstate10k`` (realestate10k_dataio.py:190-466)
returns for the scenes of tests/train_scene.py, as tests/golden/train_dataio_expected.npz.  cv2 is not installed here, so the reference
runs with a stand-in whose ``resize`` is ``dataio.resize_linear_u8``: the fixture pins the reader's draws, cameras and sampling (and the
order of its pixel operations), not cv2 itself.
Run:  python tests/golden/make_train_dataio_golden.py"""
import importlib
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_import  # noqa: E402
import train_scene  # noqa: E402

QUERY_SPARSITY = 192                     # train_realestate10k.py:78
# per seeding, the two consecutive items: scene 2 is too short, so reading it takes the reference's retry path; views = 1 on scene 0
# never retries (its query window is never empty); three views retry whenever the draws leave no room for a third frame
SEEDINGS = ((0, (0, 2)), (1, (1, 0)))
CASES = tuple((v, a, l) for v in (1, 2, 3) for a in (1, 0) for l in (1, 0))


def key(views, augment, lpips, seed, j) -> str:
    return f"v{views}.a{augment}.l{lpips}.s{seed}.i{j}"


def pack(item, gt):
    """One item's arrays: cameras, intrinsics, uv, query rgb and mask in full; context rgb as two sums and a strided probe."""
    out = {}
    assert gt is item["query"]
    for part in ("query", "context"):
        for k, v in item[part].items():
            v = np.asarray(v)
            if part == "context" and k == "rgb":
                out["context.rgb_shape"] = np.asarray(v.shape)
                out["context.rgb_sum"] = np.asarray([v.astype(np.float64).sum(), np.abs(v.astype(np.float64)).sum()])
                v = v.reshape(-1, 3)[::997]
            out[f"{part}.{k}"] = v
    return out


def main():
    from cross_attention_renderer_amd import dataio
    ref_import._install_stubs()
    for name in ("imageio", "skimage", "skimage.transform", "lpips", "h5py", "tqdm"):
        if name not in sys.modules:
            try:
                importlib.import_module(name)
            except Exception:
                sys.modules[name] = ref_import._Anything(name)
    sys.modules["cv2"].resize = lambda img, size: dataio.resize_linear_u8(np.ascontiguousarray(img), size[0], size[1])
    sys.path.insert(0, ref_import.REFERENCE_ROOT)
    ref = importlib.import_module("dataset.realestate10k_dataio")
    out = {}
    for views, augment, lpips in CASES:
        ds = ref.RealEstate10k(img_root=train_scene.img_root(), pose_root=train_scene.pose_root(), num_ctxt_views=views, num_query_views=1,
                               query_sparsity=QUERY_SPARSITY, augment=bool(augment), lpips=bool(lpips))
        for seed, ids in SEEDINGS:
            random.seed(seed)
            np.random.seed(seed)
            for j, idx in enumerate(ids):
                for k, v in pack(*ds[idx]).items():
                    out[f"{key(views, augment, lpips, seed, j)}.{k}"] = v
    path = os.path.join(HERE, "train_dataio_expected.npz")
    np.savez_compressed(path, **out)
    print("wrote", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
