"""The scenes of the training-reader tests, written from a formula (nothing but tests/golden/train_dataio_expected.npz is committed):
a RealEstate10K-style tree in a temporary directory, for tests/golden/make_train_dataio_golden.py and the tests alike.

    scenes/a_std/data.npz     300 frames stored at the working size 256 x 455
    scenes/b_raw/data.npz     300 raw frames, 360 x 640 (what the download scripts store: the reader resizes them)
    scenes/c_short/data.npz   5 frames: the reader gives up on such a scene and draws another (a retry path)
    poses.mat                 scene name -> pose table (one row of 19 numbers per frame)

300 frames leave room for three context views 93 or more frames apart.  The pixels are a sawtooth of one linear form of column, row and
frame number (so the compressed files are small and quick to write) whose three channels differ; the form is not symmetric in column and
row, and its edges make a wrong interpolation weight, flip or crop visible."""
import atexit
import os
import shutil
import tempfile

import numpy as np

N_FRAMES = 300
SCENES = (("a_std", (256, 455), N_FRAMES), ("b_raw", (360, 640), N_FRAMES), ("c_short", (256, 455), 5))
STAMP0, STAMP_STEP = 300300, 33367


def frame(shape, k: int) -> np.ndarray:
    ys, xs = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    s = 3 * xs + 2 * ys + 5 * k
    return np.stack([s % 256, (s * 3 // 2 + 80) % 256, 255 - (s // 3 + 7 * k) % 256], axis=-1).astype(np.uint8)


def pose_rows(n: int, scene: int) -> np.ndarray:
    rows = []
    for k in range(n):
        a = 0.004 * k + 0.1 * scene
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        tv = np.array([0.01 * k, 0.002 * k + 0.05 * scene, -0.004 * k])
        rows.append([STAMP0 + STAMP_STEP * k + 0.3, 0.49 + 0.0001 * k, 0.87 + 0.01 * scene, 0.5, 0.5 + 0.0001 * k, 0.0, 0.0]
                    + list(np.concatenate([R, tv[:, None]], axis=1).reshape(-1)))
    return np.asarray(rows, dtype=np.float64)


def write(root: str, scenes=SCENES) -> None:
    from scipy.io import savemat
    poses = {}
    for si, (name, shape, n) in enumerate(scenes):
        os.makedirs(os.path.join(root, "scenes", name), exist_ok=True)
        order = np.random.RandomState(si).permutation(n)                     # stored out of order: the reader sorts by time stamp
        np.savez_compressed(os.path.join(root, "scenes", name, "data.npz"),
                            **{f"{STAMP0 + STAMP_STEP * int(k)}.png": frame(shape, int(k)) for k in order})
        poses[name] = pose_rows(n, si)
    savemat(os.path.join(root, "poses.mat"), poses)


_ROOT = None


def root() -> str:
    """The tree, written once per process and removed when it ends."""
    global _ROOT
    if _ROOT is None:
        _ROOT = tempfile.mkdtemp(prefix="car_train_scene_")
        atexit.register(shutil.rmtree, _ROOT, ignore_errors=True)
        write(_ROOT)
    return _ROOT


def img_root() -> str:
    return os.path.join(root(), "scenes")


def pose_root() -> str:
    return os.path.join(root(), "poses.mat")
