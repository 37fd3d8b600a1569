"""CPU checks of the training reader (dataio.RealEstate10k, dataio.TrainLoader's host path) and of the train script's refusals.

The fixture tests/golden/train_dataio_expected.npz holds what the REFERENCE's RealEstate10k returns for the scenes of
tests/train_scene.py (tests/golden/make_train_dataio_golden.py): everything here that is compared with it is compared bit for bit."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import train_scene
from make_train_dataio_golden import CASES, QUERY_SPARSITY, SEEDINGS, key, pack

from cross_attention_renderer_amd import dataio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, "experiment_scripts", "train_realestate10k.py")
GOLDEN = os.path.join(ROOT, "tests", "golden", "train_dataio_expected.npz")


def _dataset(views, augment=True, lpips=False, query_sparsity=QUERY_SPARSITY, cls=dataio.RealEstate10k, **kw):
    return cls(img_root=train_scene.img_root(), pose_root=train_scene.pose_root(), num_ctxt_views=views, num_query_views=1,
               query_sparsity=query_sparsity, augment=bool(augment), lpips=bool(lpips), **kw)


def _same(a, b) -> bool:
    """Equal type, dtype, shape and bits."""
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    return type(a) is type(b) and a == b


def _same_batch(x, y) -> bool:
    (inp_x, gt_x), (inp_y, gt_y) = x, y
    return all(_same(inp_x[part][k], inp_y[part][k]) for part in inp_x for k in inp_x[part]) and all(_same(gt_x[k], gt_y[k]) for k in gt_x)


class _Counting(dataio.RealEstate10k):
    """Counts the calls of plan: more than one per item means a retry path was taken."""
    calls = 0

    def plan(self, idx, rng=None):
        self.calls += 1
        return super().plan(idx, rng)


@pytest.mark.parametrize("views,augment,lpips", CASES)
def test_items_equal_the_references_bit_for_bit(views, augment, lpips):
    """Both global streams seeded as the generator seeded them: every array of both consecutive items equals the reference's, so the
    number of draws an item consumes is the reference's too."""
    want = np.load(GOLDEN)
    ds = _dataset(views, augment, lpips, cls=_Counting)
    retried = {}
    for seed, ids in SEEDINGS:
        random.seed(seed)
        np.random.seed(seed)
        for j, idx in enumerate(ids):
            ds.calls = 0
            item, gt = ds[idx]
            retried[(seed, j)] = ds.calls > 1
            assert gt is item["query"]
            assert list(item["query"]) == ["rgb", "cam2world", "intrinsics", "uv", "mask"] and list(item["context"]) == ["rgb", "cam2world", "intrinsics"]
            R = 1024 if lpips else QUERY_SPARSITY
            assert item["query"]["rgb"].shape == (1, R, 3) and item["query"]["uv"].shape == (1, R, 2)
            assert item["context"]["rgb"].shape == (views, 256, 256, 3)
            assert type(item["query"]["mask"]) is (int if lpips else float)
            for part in ("query", "context"):
                for k, v in item[part].items():
                    if k != "mask":
                        assert v.dtype == torch.float32, (part, k)
            got = pack(item, gt)
            prefix = key(views, augment, lpips, seed, j)
            assert {f"{prefix}.{k}" for k in got} == {k for k in want.files if k.startswith(prefix + ".")}
            for k, v in got.items():
                w = want[f"{prefix}.{k}"]
                assert v.dtype == w.dtype and np.array_equal(v, w), f"{prefix}.{k}"
    assert retried[(0, 1)], "the short scene must send the reader down a retry path"
    if views == 1:
        assert not retried[(0, 0)] and not retried[(1, 0)]


@pytest.mark.parametrize("views,augment,lpips", [(2, 1, 1), (3, 1, 0), (1, 0, 1), (2, 0, 0)])
def test_getitem_is_the_host_chain_applied_to_plan(views, augment, lpips):
    ds = _dataset(views, augment, lpips)
    for idx in (0, 1):
        random.seed(7 + idx)
        np.random.seed(7 + idx)
        item, _ = ds[idx]
        random.seed(7 + idx)
        np.random.seed(7 + idx)
        plan = ds.plan(idx)
        assert all(f.dtype == np.uint8 and f.shape in ((256, 455, 3), (360, 640, 3)) for f in plan["frames"])       # raw stored frames
        assert len(plan["frames"]) == len(plan["records"]) == 1 + views
        assert all(set(r) >= {"resize360", "flip", "py", "px"} for r in plan["records"])
        again, _ = ds.apply_plan(plan)
        for part in item:
            for k in item[part]:
                assert _same(item[part][k], again[part][k]), (part, k)
        # a private pair of generators gives the same item whatever the global streams hold, and leaves them alone
        state = random.getstate(), np.random.get_state()[1].copy()
        a = ds.apply_plan(ds.plan(idx, dataio.PrivateStreams([3, idx])))[0]
        random.seed(99)
        b = ds.apply_plan(ds.plan(idx, dataio.PrivateStreams([3, idx])))[0]
        random.setstate(state[0])
        assert all(_same(a[part][k], b[part][k]) for part in a for k in a[part])
        assert np.array_equal(np.random.get_state()[1], state[1])


def test_flip_crop_resize_by_hand():
    """One augmented frame against resize_linear_u8 on the explicitly sliced array, and the camera algebra that goes with it."""
    raw = train_scene.frame((256, 455), 17)
    rec = {"resize360": False, "augment": True, "flip": True, "py": 5, "px": 12}
    want = dataio.resize_linear_u8(np.ascontiguousarray(raw[:, 99:355][:, ::-1][5:251, 12:244]), 256, 256).astype(np.float32) / 127.5 - 1
    got = dataio.frame_pixels(raw, rec)
    assert got.dtype == np.float32 and got.shape == (256, 256, 3) and np.array_equal(got, want)
    # mirrored first, cropped second: the crop is symmetric, so the same columns are read from the right
    assert np.array_equal(got, dataio.resize_linear_u8(np.ascontiguousarray(raw[5:251, 99 + 12:355 - 12][:, ::-1]), 256, 256).astype(np.float32) / 127.5 - 1)
    raw360 = train_scene.frame((360, 640), 3)
    want = dataio.square_crop_img(dataio.resize_linear_u8(raw360, 455, 256)).astype(np.float32) / 127.5 - 1
    assert np.array_equal(dataio.frame_pixels(raw360, {"resize360": True, "augment": False, "flip": False, "py": 0, "px": 0}), want)

    class Fixed:                                               # draws that give flip, py = 5, px = 12
        class np:
            seq = iter([0.1, 0.2, 5, 0.3, 12])
            uniform = staticmethod(lambda a, b: next(Fixed.np.seq))
            randint = staticmethod(lambda a, b: next(Fixed.np.seq))
    ds = _dataset(2, augment=True, query_sparsity=None)
    pose = ds.all_pose["a_std"]
    stamp = int(round(pose[17, 0]))
    rec, K, c2w, pixels, mask = ds._frame_plan((256, 455, 3), pose, stamp, Fixed, query=True)
    assert (rec["flip"], rec["py"], rec["px"]) == (True, 5, 12) and pixels is None and mask == 0.0
    cam = dataio.parse_pose(pose, stamp)
    assert np.array_equal(c2w, cam.c2w_mat @ np.diag([-1.0, 1.0, 1.0, 1.0]))
    assert K[0, 0] == cam.intrinsics[0, 0] * 455 * (256 / 232) and K[1, 1] == cam.intrinsics[1, 1] * 256 * (256 / 246)
    assert K[0, 2] == cam.intrinsics[0, 2] * 455 / (455 / 256) and K[1, 2] == cam.intrinsics[1, 2] * 256            # the principal point stays


def test_ray_sampling_forms():
    ds = _dataset(2, augment=True, lpips=True)
    seen = set()
    for s in range(12):
        random.seed(s)
        np.random.seed(s)
        plan = ds.plan(0)
        pix, mask = plan["pixels"][0], plan["query"]["mask"]
        seen.add(mask)
        assert len(pix) == 1024 and pix.max() < 65536
        if mask:                                               # one 32 x 32 patch, row-major
            y0, x0 = divmod(int(pix[0]), 256)
            assert y0 <= 223 and x0 <= 223
            assert np.array_equal(pix.reshape(32, 32), (y0 + np.arange(32))[:, None] * 256 + x0 + np.arange(32)[None])
        else:
            assert len(set(pix.tolist())) == 1024
        assert torch.equal(plan["query"]["uv"][0], ds.uv[pix])
    assert seen == {0, 1}


def test_host_loader_is_reproducible_and_drops_the_last_partial_batch():
    ds = _dataset(2, augment=True)
    assert len(ds) == 3
    one = list(dataio.TrainLoader(ds, batch_size=2, seed=5, num_workers=1))
    eight = list(dataio.TrainLoader(ds, batch_size=2, seed=5, num_workers=8))
    assert len(one) == len(eight) == 1 == len(dataio.TrainLoader(ds, batch_size=2))                                   # 3 scenes: one batch of 2
    assert all(_same_batch(x, y) for x, y in zip(one, eight))
    inp, gt = one[0]
    assert inp["context"]["rgb"].shape == (2, 2, 256, 256, 3) and inp["query"]["rgb"].shape == (2, 1, QUERY_SPARSITY, 3)
    assert inp["query"]["uv"].shape == (2, 1, QUERY_SPARSITY, 2) and inp["query"]["mask"].shape == (2,) and inp["query"]["mask"].dtype == torch.float64
    assert all(_same(gt[k], inp["query"][k]) for k in gt)
    other = list(dataio.TrainLoader(ds, batch_size=2, seed=6, num_workers=8))
    assert not _same_batch(one[0], other[0])
    loader = dataio.TrainLoader(ds, batch_size=1, seed=5, num_workers=40)
    assert loader.num_workers == 16
    first, second = list(loader), list(loader)                 # two epochs: both whole, shuffled and drawn anew
    assert len(first) == len(second) == 3 and not all(_same_batch(x, y) for x, y in zip(first, second))
    with pytest.raises(ValueError):
        dataio.TrainLoader(ds, batch_size=2, device="cpu")


def test_vis_reader_still_refuses_training_options():
    for kw in ({"augment": True}, {"query_sparsity": 192}, {"lpips": True}):
        with pytest.raises(ValueError, match="training-time"):
            dataio.RealEstate10kVis(train_scene.img_root(), train_scene.pose_root(), 2, 1, **kw)
    assert dataio.ACIDVis is dataio.RealEstate10kVis and not hasattr(dataio, "ACID")


def test_train_script_refusals_need_no_device(tmp_path):
    base = [sys.executable, TRAIN, "--experiment_name", "t", "--logging_root", str(tmp_path)]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")           # a device that is opened anyway fails differently
    out = subprocess.run(base + ["--data_root", str(tmp_path)], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode != 0 and "--pose_root" in out.stderr and "Traceback" not in out.stderr, out.stderr
    out = subprocess.run(base + ["--data_root", str(tmp_path), "--pose_root", "poses.mat", "--depth"], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode != 0 and "--depth" in out.stderr and "--lpips" in out.stderr and "Traceback" not in out.stderr, out.stderr
    out = subprocess.run([sys.executable, TRAIN, "--help"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "--no_data_aug" in out.stdout and "--num_workers" in out.stdout
