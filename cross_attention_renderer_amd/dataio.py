"""RealEstate10K / ACID scene reader for the render scripts.

Behaviour of the reference's ``dataset/realestate10k_dataio.py`` (``Camera`` :61-73, ``unnormalize_intrinsics`` :75-79,
``parse_pose_file`` :82-91, ``get_camera_pose`` :104-188), written against its observable results: the committed fixture
``tests/golden/dataio_scene`` holds a small scene and what the reference returns for it (``tests/golden/make_dataio_golden.py``).

On disk a scene is a directory with one ``*.npz`` whose keys are ``<timestamp>.<ext>`` -> decoded uint8 frame, and a camera
file ``<pose_dir>/<scene name>.txt``: one header line, then per frame
``timestamp fx fy cx cy _ _ r00 r01 r02 t0 r10 r11 r12 t1 r20 r21 r22 t2`` with intrinsics normalised by the image size
and a 3x4 world-to-camera matrix."""
from __future__ import annotations

import random
from pathlib import Path
from typing import Dict

import numpy as np
import torch

# The reference hard-codes the frame geometry its intrinsics refer to (realestate10k_dataio.py:124-128): focal lengths are
# scaled by the un-cropped 256 x 456 frame, principal points by the square 256 x 256 crop.
FRAME_H, FRAME_W = 256, 456
MAX_FRAMES = 128


class Camera:
    """One line of a camera file: 4x4 normalised intrinsics, world-to-camera and camera-to-world matrices (float64)."""

    def __init__(self, entry):
        fx, fy, cx, cy = entry[1:5]
        self.intrinsics = np.array([[fx, 0.0, cx, 0.0], [0.0, fy, cy, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
        self.w2c_mat = np.eye(4)
        self.w2c_mat[:3, :] = np.asarray(entry[7:19], dtype=np.float64).reshape(3, 4)
        self.c2w_mat = np.linalg.inv(self.w2c_mat)


def unnormalize_intrinsics(intrinsics: np.ndarray, h: int, w: int) -> np.ndarray:
    out = intrinsics.copy()
    out[0] *= w
    out[1] *= h
    return out


def parse_pose_file(path) -> Dict[int, Camera]:
    """timestamp -> Camera; the first line of the file is a header (the video URL)."""
    cams: Dict[int, Camera] = {}
    with open(path, "r") as f:
        for i, line in enumerate(f):
            if i == 0:
                continue
            entry = [float(x) for x in line.split()]
            if entry:
                cams[int(entry[0])] = Camera(entry)
    return cams


def _pixel_intrinsics(cam: Camera) -> np.ndarray:
    K = unnormalize_intrinsics(cam.intrinsics, FRAME_H, FRAME_W)
    short = min(FRAME_H, FRAME_W)
    K[0, 2] = K[0, 2] / (FRAME_W / short)
    K[1, 2] = K[1, 2] / (FRAME_H / short)
    return K


def get_camera_pose(scene_path, all_pose_dir, uv: torch.Tensor, views: int = 1) -> Dict[str, Dict[str, torch.Tensor]]:
    """The model input of the trajectory render script: context = first / middle / last of the first 129 frames (by ``views``),
    queries = frames 1 .. 127 with their ground-truth images; rgb in [-1, 1]; all tensors float32 with a leading batch of 1."""
    scene_path = Path(scene_path)
    data = np.load(sorted(scene_path.glob("*.npz"))[0])
    names = list(data.keys())
    stamps = np.array([int(n.split(".")[0]) for n in names])
    order = np.argsort(stamps)
    names = [names[i] for i in order]
    stamps = stamps[order]
    cams = parse_pose_file(Path(all_pose_dir) / (scene_path.name + ".txt"))

    def frame(i):
        cam = cams[int(stamps[i])]
        return data[names[i]].astype(np.float32) / 127.5 - 1, cam.c2w_mat, _pixel_intrinsics(cam)

    n = len(names)
    n_render = min(MAX_FRAMES, n)
    last = min(n - 1, MAX_FRAMES)
    if views == 1:
        ctx_ids = [0]
    elif views == 2:
        ctx_ids = [0, last]
    elif views == 3:
        ctx_ids = [0, last // 2, last]
    else:
        raise ValueError(f"views must be 1, 2 or 3 (got {views})")

    def pack(ids):
        rgb, c2w, K = zip(*(frame(i) for i in ids)) if ids else ((), (), ())
        as_t = lambda arrs: torch.from_numpy(np.stack(arrs).astype(np.float32))[None] if arrs else torch.zeros(1, 0)
        return {"rgb": as_t(rgb), "cam2world": as_t(c2w), "intrinsics": as_t(K)}

    query = pack(list(range(1, n_render)))
    query["uv"] = uv.view(-1, 2)[None, None].expand(1, n_render - 1, -1, -1)
    return {"query": query, "context": pack(ctx_ids)}


# ----------------------------------------------------------------------------------------------------------------------
# Evaluation items (reference RealEstate10kVis / ACIDVis, realestate10k_dataio.py:469-719, acid_dataio.py:504-): one scene ->
# (model_input, query) with the first / last (/ middle) of the first 129 frames as context and one random in-between frame as query.
# ----------------------------------------------------------------------------------------------------------------------
def parse_pose(pose_rows: np.ndarray, timestep: int) -> Camera:
    """The camera of frame ``timestep`` from the rows of a ``.mat`` pose table (one row per frame, same 19 numbers as a line of a
    camera file; timestamps are matched after rounding, realestate10k_dataio.py:95-101)."""
    mask = (np.around(pose_rows[:, :1]) == timestep)[:, 0]
    return Camera(pose_rows[mask][0])


def square_crop_img(img: np.ndarray) -> np.ndarray:
    """Centre crop to the shorter side (utils/data_util.py:116-121; for an odd difference the crop is one pixel short, as there)."""
    m = int(np.amin(img.shape[:2]))
    c = np.array(img.shape[:2]) // 2
    return img[c[0] - m // 2:c[0] + m // 2, c[1] - m // 2:c[1] + m // 2]


def _linear_coefs(n_dst: int, n_src: int):
    """Source index and the two 11-bit fixed-point weights of every destination index, as OpenCV's ``resize`` computes them for
    INTER_LINEAR on 8-bit images: centre-aligned coordinate ``(d + 0.5) * scale - 0.5`` in float32, clamped at both ends,
    weights rounded to 1/2048."""
    scale = 1.0 / (float(n_dst) / float(n_src))
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    i0 = np.floor(f).astype(np.int64)
    f = f - i0.astype(np.float32)
    lo, hi = i0 < 0, i0 >= n_src - 1
    f = np.where(lo | hi, np.float32(0), f)
    i0 = np.where(lo, 0, np.where(hi, n_src - 1, i0))
    i1 = np.minimum(i0 + 1, n_src - 1)
    w1 = np.rint(f.astype(np.float32) * np.float32(2048)).astype(np.int64)
    w0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)
    return i0, i1, w0, w1


def resize_linear_u8(img: np.ndarray, width: int, height: int) -> np.ndarray:
    """``cv2.resize(img, (width, height))`` (INTER_LINEAR) for a uint8 H x W x C image, restated from OpenCV's fixed-point path
    (imgproc/resize.cpp: 11-bit coefficients, horizontal pass in int32, vertical pass ``((b0 (S0 >> 4)) >> 16) + ((b1 (S1 >> 4))
    >> 16) + 2) >> 2``).  The reference resizes its 360-line frames this way when an item is read (realestate10k_dataio.py:606-607).
    cv2 is not installed in this image, so the restatement is unpinned against cv2 itself (tests check it against float bilinear
    interpolation to one grey level)."""
    if img.dtype != np.uint8 or img.ndim != 3:
        raise ValueError("resize_linear_u8 expects a uint8 H x W x C image")
    x0, x1, a0, a1 = _linear_coefs(width, img.shape[1])
    y0, y1, b0, b1 = _linear_coefs(height, img.shape[0])
    src = img.astype(np.int64)
    rows = src[:, x0] * a0[None, :, None] + src[:, x1] * a1[None, :, None]               # horizontal pass: values x 2048
    out = (((b0[:, None, None] * (rows[y0] >> 4)) >> 16) + ((b1[:, None, None] * (rows[y1] >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


class RealEstate10kVis:
    """Evaluation dataset of the reference's eval scripts (eval_realestate10k.py:101-105, eval_acid.py): ``img_root`` holds one
    directory per scene with a ``*.npz`` of frames, ``pose_root`` is a ``.mat`` file mapping scene name -> pose table.  The
    download scripts store raw 360-line frames; like the reference (realestate10k_dataio.py:606-607) the reader resizes such a frame
    to the working size 256 x 455 (``resize_linear_u8``: OpenCV's INTER_LINEAR restated) before the centre crop to 256 x 256."""

    H, W = 256, 455

    def __init__(self, img_root, pose_root, num_ctxt_views: int, num_query_views: int = 1, query_sparsity=None, max_num_scenes=None,
                 square_crop: bool = True, augment: bool = False, lpips: bool = False):
        from scipy.io import loadmat
        if augment or query_sparsity is not None or lpips:
            raise ValueError("RealEstate10kVis here is the evaluation reader: augment / query_sparsity / lpips are training-time options")
        if num_ctxt_views not in (1, 2, 3):
            raise ValueError("More than 3 context views not supported")
        self.num_ctxt_views = num_ctxt_views
        self.all_pose = loadmat(str(pose_root))
        self.all_scenes = sorted(p for p in Path(img_root).glob("*/") if p.is_dir())
        if max_num_scenes:
            self.all_scenes = self.all_scenes[:max_num_scenes]
        self.square_crop = square_crop
        short = min(self.H, self.W)
        self.xscale, self.yscale = self.W / short, self.H / short
        if square_crop:
            ys, xs = torch.meshgrid(torch.arange(0, short), torch.arange(0, short), indexing="ij")
        else:
            ys, xs = torch.meshgrid(torch.arange(0, self.H), torch.arange(0, self.W), indexing="ij")
        self.uv = torch.stack([xs.float(), ys.float()], dim=-1).reshape(-1, 2)          # (x = column, y = row), row-major

    def __len__(self) -> int:
        return len(self.all_scenes)

    def _frame(self, data, name, pose, stamp):
        rgb = data[name]
        if rgb.shape[0] == 360:
            rgb = resize_linear_u8(np.ascontiguousarray(rgb), self.W, self.H)
        if self.square_crop:
            rgb = square_crop_img(rgb)
        cam = parse_pose(pose, stamp)
        K = unnormalize_intrinsics(cam.intrinsics, self.H, self.W)
        if self.square_crop:
            K[0, 2] = K[0, 2] / self.xscale
            K[1, 2] = K[1, 2] / self.yscale
        return rgb.astype(np.float32) / 127.5 - 1, K, cam.c2w_mat

    def __getitem__(self, idx):
        import random
        retry = lambda: self.__getitem__(random.randint(0, len(self.all_scenes) - 1))       # the reference's answer to a bad scene
        scene = self.all_scenes[idx]
        files = sorted(scene.glob("*.npz"))
        if scene.name not in self.all_pose or not files:
            return retry()
        pose = self.all_pose[scene.name]
        try:
            data = np.load(files[0])
        except Exception:
            return retry()
        names = list(data.keys())
        if len(names) <= 10:
            return retry()
        stamps = np.array([int(n.split(".")[0]) for n in names])
        order = np.argsort(stamps)
        names, stamps = np.array(names)[order], stamps[order]
        end = min(len(names) - 1, MAX_FRAMES)
        id_feat = {1: [0], 2: [0, end], 3: [0, end // 2, end]}[self.num_ctxt_views]
        candidates = [i for i in range(0, end) if np.abs(np.array(id_feat) - i).min() > 10]
        if not candidates:
            return retry()
        q = random.choice(candidates)
        rgb, K, c2w = self._frame(data, names[q], pose, stamps[q])
        query = {"rgb": torch.from_numpy(rgb.reshape(-1, 3)[None]).float(), "cam2world": torch.from_numpy(c2w[None]).float(),
                 "intrinsics": torch.from_numpy(K[None]).float(), "uv": self.uv[None].float(), "mask": 0.0}
        ctx = [self._frame(data, names[i], pose, stamps[i]) for i in id_feat]
        context = {"rgb": torch.from_numpy(np.stack([c[0] for c in ctx])).float(),
                   "cam2world": torch.from_numpy(np.stack([c[2] for c in ctx])).float(),
                   "intrinsics": torch.from_numpy(np.stack([c[1] for c in ctx])).float()}
        return {"query": query, "context": context}, query


ACIDVis = RealEstate10kVis          # acid_dataio.py:504- is the same reader over the ACID download (eval_acid.py)


# ----------------------------------------------------------------------------------------------------------------------
# Training items (reference RealEstate10k, realestate10k_dataio.py:24-59, 190-466): random context frames, a query frame near them,
# per-frame augmentation, sparse ray sampling.  An item is made in two halves so that the pixel work can run on the device:
# ``plan`` makes every random draw and all camera algebra and touches no pixel; ``apply_plan`` (host) or ``TrainLoader`` (device,
# csrc/car_frames.hip) runs the pixel chain of the plan.  Draws are made in the reference's order and number from the reference's two
# global streams, so seeding ``random`` and ``np.random`` reproduces its items (tests/golden/train_dataio_expected.npz).
# ----------------------------------------------------------------------------------------------------------------------
SIDE = 256                         # the side every training frame ends at (augment's resize, realestate10k_dataio.py:52)
PATCH = 32                         # lpips: side of the ray patch (realestate10k_dataio.py:387)
LPIPS_RAYS = 1024                  # lpips: rays per query frame, patch or not (realestate10k_dataio.py:397)


class GlobalStreams:
    """The reference's random sources: the ``random`` module and ``np.random``'s global state."""
    py = random
    np = np.random


class PrivateStreams:
    """A private pair of the same two generators, for a loader whose worker threads must not share (or disturb) the global ones."""

    def __init__(self, seed):
        a, b = (int(x) for x in np.random.SeedSequence(seed).generate_state(2))
        self.py, self.np = random.Random(a), np.random.RandomState(b)


def _draw_augment(rs):
    """augment's draws (realestate10k_dataio.py:33-49): flip, then the row crop py, then the column crop px."""
    flip = bool(rs.uniform(0, 1) < 0.5)
    py = int(rs.randint(1, 32)) if rs.uniform(0, 1) < 0.5 else 0
    px = int(rs.randint(1, 32)) if rs.uniform(0, 1) < 0.5 else 0
    return flip, py, px


def frame_pixels(raw: np.ndarray, rec: dict, square_crop: bool = True, size=(256, 455)) -> np.ndarray:
    """The host pixel chain of one frame: raw stored uint8 frame -> float32 image in [-1, 1] (realestate10k_dataio.py:355-374)."""
    rgb = raw
    if rec["resize360"]:
        rgb = resize_linear_u8(np.ascontiguousarray(rgb), size[1], size[0])
    if square_crop:
        rgb = square_crop_img(rgb)
    if rec["augment"]:
        if rec["flip"]:
            rgb = rgb[:, ::-1, :]
        if rec["py"]:
            rgb = rgb[rec["py"]:-rec["py"], :, :]
        if rec["px"]:
            rgb = rgb[:, rec["px"]:-rec["px"], :]
        rgb = resize_linear_u8(np.ascontiguousarray(rgb), SIDE, SIDE)
    return rgb.astype(np.float32) / 127.5 - 1


class RealEstate10k:
    """Training dataset of the reference's train script (train_realestate10k.py:74-79): ``img_root`` holds one directory per scene with
    a ``*.npz`` of frames, ``pose_root`` is a ``.mat`` file mapping scene name -> pose table.  ``ds[i]`` is the reference's item
    ``({'query', 'context'}, query)``; cv2's resize is ``resize_linear_u8`` (its restatement, unpinned against cv2 itself)."""

    H, W = 256, 455

    def __init__(self, img_root, pose_root, num_ctxt_views, num_query_views, query_sparsity=None, max_num_scenes=None,
                 square_crop: bool = True, augment: bool = True, lpips: bool = False):
        from scipy.io import loadmat
        if num_ctxt_views not in (1, 2, 3):
            raise ValueError("More than 3 context views not supported")
        self.num_ctxt_views, self.num_query_views, self.query_sparsity = num_ctxt_views, num_query_views, query_sparsity
        self.all_pose = loadmat(str(pose_root))
        self.lpips, self.augment, self.square_crop = lpips, augment, square_crop
        self.all_scenes = sorted(Path(img_root).glob("*/"))
        if max_num_scenes:
            self.all_scenes = self.all_scenes[:max_num_scenes]
        short = min(self.H, self.W)
        self.xscale, self.yscale = self.W / short, self.H / short
        if square_crop:
            ys, xs = torch.meshgrid(torch.arange(0, short), torch.arange(0, short), indexing="ij")
        else:
            ys, xs = torch.meshgrid(torch.arange(0, self.H), torch.arange(0, self.W), indexing="ij")
        self.uv = torch.stack([xs.float(), ys.float()], dim=-1).reshape(-1, 2)          # (x = column, y = row), row-major

    def __len__(self) -> int:
        return len(self.all_scenes)

    # ---- first half: draws and cameras ------------------------------------------------------------------------------------------
    def _frame_plan(self, raw_shape, pose, stamp, rng, query: bool):
        """One frame's record, intrinsics and pose, in the reference's order of draws (realestate10k_dataio.py:357-405)."""
        h, w = raw_shape[:2]
        rec = {"resize360": h == 360, "augment": bool(self.augment), "flip": False, "py": 0, "px": 0}
        if rec["resize360"]:
            h, w = self.H, self.W
        if self.square_crop:
            m = min(h, w)
            h, w = 2 * (m // 2), 2 * (m // 2)                # square_crop_img: an odd side comes out one pixel short
        cam = parse_pose(pose, stamp)
        K = unnormalize_intrinsics(cam.intrinsics, self.H, self.W)
        if self.square_crop:
            K[0, 2] = K[0, 2] / self.xscale
            K[1, 2] = K[1, 2] / self.yscale
        c2w = cam.c2w_mat
        if self.augment:
            rec["flip"], rec["py"], rec["px"] = _draw_augment(rng.np)
            if rec["flip"]:
                c2w = c2w @ np.array([[-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
            K[0, 0] = K[0, 0] * (SIDE / (w - 2 * rec["px"]))  # the principal point is left alone, as in the reference
            K[1, 1] = K[1, 1] * (SIDE / (h - 2 * rec["py"]))
            h, w = SIDE, SIDE
        rec["out_hw"] = (h, w)
        pixels, mask = None, 0.0
        if query and self.query_sparsity is not None:
            n = self.uv.shape[0]
            if self.lpips:
                mask = rng.py.randint(0, 1)
                if mask:                                     # one 32 x 32 patch of the 256 x 256 frame at a random corner
                    x_off, y_off = rng.np.randint(0, SIDE - PATCH), rng.np.randint(0, SIDE - PATCH)
                    pixels = ((y_off + np.arange(PATCH))[:, None] * SIDE + (x_off + np.arange(PATCH))[None, :]).reshape(-1)
                else:
                    pixels = rng.np.permutation(n)[:LPIPS_RAYS]
            else:
                pixels = rng.np.permutation(n)[:self.query_sparsity]
        return rec, K, c2w, pixels, mask

    def plan(self, idx, rng=None):
        """Every random draw and all camera algebra of item ``idx``: the raw stored uint8 frames (query frames first, then context) with
        a record per frame (needs-360-resize, flip, py, px), the selected pixel indices of the query frames, cameras, uv and mask.  No
        pixel is touched.  ``rng=None`` draws from the global ``random`` / ``np.random`` streams as the reference does; otherwise an
        object with ``.py`` (``random.Random``) and ``.np`` (``np.random.RandomState``), e.g. ``PrivateStreams(seed)``."""
        rng = GlobalStreams if rng is None else rng
        retry = lambda: self.plan(rng.py.randint(0, len(self.all_scenes) - 1), rng)       # the reference's answer to a bad scene
        scene = self.all_scenes[idx]
        files = sorted(scene.glob("*.npz"))
        if scene.name not in self.all_pose:
            return retry()
        pose = self.all_pose[scene.name]
        if not files:
            return retry()
        try:
            data = np.load(files[0])
        except Exception:
            return retry()
        with data:
            names = list(data.keys())
            if len(names) <= 10:
                return retry()
            stamps = np.array([int(n.split(".")[0]) for n in names])
            order = np.argsort(stamps)
            names, stamps = np.array(names)[order], stamps[order]
            num_frames = len(names)
            rng.np.randint(low=-1, high=2)                                               # the reference's unused `shift`
            candidates = np.arange(0, num_frames - 1)
            if len(candidates) < self.num_ctxt_views:
                return retry()
            id_feats = []
            for _ in range(self.num_ctxt_views):
                if len(candidates) == 0:
                    return retry()
                id_feat = rng.np.choice(candidates, size=1, replace=False)
                candidates = candidates[(candidates < (id_feat - 92)) | (candidates > (id_feat + 92))]
                id_feats.append(id_feat.item())
            id_feat = np.array(id_feats)
            if self.num_ctxt_views in (1, 2):
                low, high = max(np.min(id_feat) - 64, 0), min(np.max(id_feat) + 64, num_frames - 1)
            else:
                low, high = np.min(id_feat) + 64, np.max(id_feat) - 64
            if high <= low:
                return retry()
            id_render = rng.np.randint(low=low, high=high, size=self.num_query_views)
            frames, records = [], []
            parts = {"query": ([], [], [], 0.0), "context": ([], [], [], 0.0)}
            pixels = []
            for part, ids in (("query", id_render), ("context", id_feat)):
                Ks, c2ws, uvs, mask = parts[part]
                for i in ids:
                    raw = data[names[i]]
                    rec, K, c2w, pix, m = self._frame_plan(raw.shape, pose, stamps[i], rng, query=part == "query")
                    frames.append(raw)
                    records.append(rec)
                    Ks.append(K)
                    c2ws.append(c2w)
                    if part == "query":
                        pixels.append(pix)
                        uvs.append(self.uv if pix is None else self.uv[pix])
                        mask = m                              # the reference keeps the LAST query frame's mask
                parts[part] = (Ks, c2ws, uvs, mask)
        pack = lambda arrs: torch.from_numpy(np.stack(arrs)).float()
        qK, qc, quv, qmask = parts["query"]
        cK, cc, _, _ = parts["context"]
        return {"frames": frames, "records": records, "pixels": pixels, "num_query": len(id_render),
                "query": {"cam2world": pack(qc), "intrinsics": pack(qK), "uv": torch.stack(quv).float(), "mask": qmask},
                "context": {"cam2world": pack(cc), "intrinsics": pack(cK)}}

    # ---- second half: pixels, on the host ---------------------------------------------------------------------------------------
    def apply_plan(self, plan):
        """The host pixel chain applied to a plan: the reference's item ``({'query', 'context'}, query)``."""
        nq = plan["num_query"]
        imgs = [frame_pixels(f, r, self.square_crop, (self.H, self.W)) for f, r in zip(plan["frames"], plan["records"])]
        q_rgb = []
        for img, pix in zip(imgs[:nq], plan["pixels"]):
            flat = img.reshape(-1, 3)
            q_rgb.append(flat if pix is None else flat[pix])
        query = dict(plan["query"], rgb=torch.from_numpy(np.stack(q_rgb)).float())
        query = {k: query[k] for k in ("rgb", "cam2world", "intrinsics", "uv", "mask")}
        context = {"rgb": torch.from_numpy(np.stack(imgs[nq:])).float(), "cam2world": plan["context"]["cam2world"],
                   "intrinsics": plan["context"]["intrinsics"]}
        return {"query": query, "context": context}, query

    def __getitem__(self, idx):
        return self.apply_plan(self.plan(idx))


# ----------------------------------------------------------------------------------------------------------------------
# The loader: what the reference gets from DataLoader(shuffle=True, drop_last=True, num_workers=8) (train_realestate10k.py:80-81), with
# the pixel chain on the device.  Worker threads make plans; one assembler thread lays a batch's raw frames, records and pixel indices
# into a pinned staging buffer, uploads it with one copy and launches the two stages on a stream of its own; the consumer's stream
# waits on the batch's event.  No step waits on the host except where a pinned buffer is reused (its own event).
# ----------------------------------------------------------------------------------------------------------------------
MAX_WORKERS = 16

# struct car_frame_rec (include/car_hip.h)
FRAME_REC = np.dtype([("src_off", "<i8"), ("dst_off", "<i8"), ("idx_off", "<i8"), ("src_h", "<i4"), ("src_w", "<i4"), ("src_pitch", "<i4"),
                      ("x0", "<i4"), ("y0", "<i4"), ("rw", "<i4"), ("rh", "<i4"), ("flip", "<i4"), ("dst_w", "<i4"), ("dst_h", "<i4"),
                      ("win_x0", "<i4"), ("win_w", "<i4"), ("n_idx", "<i4"), ("reserved", "<i4")])
CROP_X0 = 455 // 2 - SIDE // 2      # 99: the first column the centre crop keeps of a 256 x 455 frame


def frame_tables() -> np.ndarray:
    """The coefficient tables of csrc/car_frames.hip as one int32 array (include/car_hip.h): a slot of {i0, i1, w0, w1} entries for every
    resize the chain can ask for, from ``_linear_coefs``, then the 256 float32 values ``v / 127.5 - 1`` as numpy computes them."""
    from . import _lib
    lib = _lib.api()
    out = np.zeros(lib.car_frames_table_ints(), dtype=np.int32)
    pairs = [(SIDE - 2 * p, SIDE) for p in range(32)] + [(360, 256), (640, 455)]
    for n_src, n_dst in pairs:
        slot = lib.car_frames_table_slot(n_src, n_dst)
        if slot < 0:
            raise RuntimeError(f"libcar_hip.so has no table slot for {n_src} -> {n_dst}")
        at = slot * 512 * 4
        out[at:at + 4 * n_dst] = np.stack(_linear_coefs(n_dst, n_src), axis=-1).astype(np.int32).reshape(-1)
    out[-256:] = (np.arange(256, dtype=np.uint8).astype(np.float32) / 127.5 - 1).view(np.int32)
    return out


def stage_records(shapes, records, pixels, frame_offs, scratch_off):
    """The records of both stages for a batch of frames (all of them ending at 256 x 256): ``shapes[i]`` the stored shape of frame i at
    byte ``frame_offs[i]`` of the device buffer, ``records[i]`` its plan record, ``pixels[i]`` its pixel index list or None.  Stage A
    resizes every 360-line frame to its 256 x 256 centre window at ``scratch_off`` onwards (uint8); stage B reads that window, or a
    stored 256 x 455 frame's, mirrored and cropped as the record says.  Returns (recs_a, recs_b, idx): stage B's dst_off counts floats
    from the start of one output array that holds the frames in order, dense ones as 65536 x 3, sparse ones as n x 3."""
    n = len(shapes)
    recs_a, recs_b = np.zeros(sum(r["resize360"] for r in records), FRAME_REC), np.zeros(n, FRAME_REC)
    idx, n_a, dst, n_idx = [], 0, 0, 0
    for i, (shape, rec, pix) in enumerate(zip(shapes, records, pixels)):
        b = recs_b[i]
        if rec["resize360"]:
            if tuple(shape) != (360, 640, 3):
                raise ValueError(f"the device path reads 360 x 640 raw frames (got {tuple(shape)})")
            a = recs_a[n_a]
            a["src_off"], a["src_h"], a["src_w"], a["src_pitch"] = frame_offs[i], 360, 640, 640 * 3
            a["x0"], a["y0"], a["rw"], a["rh"], a["dst_w"], a["dst_h"] = 0, 0, 640, 360, 455, 256
            a["win_x0"], a["win_w"], a["dst_off"] = CROP_X0, SIDE, n_a * SIDE * SIDE * 3
            b["src_off"], b["src_h"], b["src_w"], b["src_pitch"] = scratch_off + n_a * SIDE * SIDE * 3, SIDE, SIDE, SIDE * 3
            x0 = 0
            n_a += 1
        else:
            if tuple(shape) != (256, 455, 3):
                raise ValueError(f"the device path reads stored 256 x 455 frames or raw 360 x 640 ones (got {tuple(shape)})")
            b["src_off"], b["src_h"], b["src_w"], b["src_pitch"] = frame_offs[i], 256, 455, 455 * 3
            x0 = CROP_X0
        py, px = (rec["py"], rec["px"]) if rec["augment"] else (0, 0)
        b["x0"], b["y0"], b["rw"], b["rh"] = x0 + px, py, SIDE - 2 * px, SIDE - 2 * py
        b["flip"] = int(rec["augment"] and rec["flip"])
        b["dst_w"], b["dst_h"], b["win_x0"], b["win_w"], b["dst_off"] = SIDE, SIDE, 0, SIDE, dst
        if pix is None:
            dst += SIDE * SIDE * 3
        else:
            b["idx_off"], b["n_idx"] = n_idx, len(pix)
            idx.append(np.asarray(pix, dtype=np.int32))
            n_idx += len(pix)
            dst += -(-len(pix) * 3 // 4) * 4                 # every image's output starts on a multiple of 4 floats
    return recs_a, recs_b, (np.concatenate(idx) if idx else np.zeros(0, np.int32))


def _align(n: int, a: int = 256) -> int:
    return -(-n // a) * a


class TrainLoader:
    """Batches of ``dataset`` (a ``RealEstate10k``) for the training loop: shuffled per epoch from ``seed``, the last partial batch
    dropped, ``num_workers`` threads (capped at 16) making the plans with a private rng per (seed, epoch, index), ``prefetch`` batches
    prepared ahead.  Iterating yields one epoch of ``(model_input, gt)``.

    ``device=None``: the host path — every item is the dataset's host chain, collated by ``torch.utils.data.default_collate``.
    With a device, the raw uint8 frames of a batch are uploaded in one copy and the pixel chain runs there (csrc/car_frames.hip); the
    batch is on the device, bit-identical to the host path's, its camera tensors placed as ``harness.to_device(..., cameras=)`` does."""

    def __init__(self, dataset, batch_size: int, seed: int = 0, num_workers: int = 8, device=None, cameras: str = "host", prefetch: int = 2):
        if cameras not in ("host", "gpu", "device"):
            raise ValueError("cameras must be 'host', 'gpu' or 'device'")
        if not 1 <= prefetch <= 2:
            raise ValueError("prefetch must be 1 or 2 batches")
        if batch_size < 1 or num_workers < 1:
            raise ValueError("batch_size and num_workers must be positive")
        self.dataset, self.batch_size, self.seed, self.cameras, self.prefetch = dataset, batch_size, int(seed), cameras, prefetch
        self.num_workers = min(int(num_workers), MAX_WORKERS)
        self.device = None if device is None else torch.device(device)
        self.epoch = 0
        self._dev = None
        if self.device is not None:
            if self.device.type != "cuda":
                raise ValueError("TrainLoader's device path needs a GPU; device=None is the host path")
            if not dataset.square_crop:
                raise ValueError("the device path covers square_crop=True, the reference's training setting")

    def __len__(self) -> int:
        return len(self.dataset) // self.batch_size

    def batch_indices(self, epoch: int):
        perm = np.random.RandomState([self.seed & 0xFFFFFFFF, epoch]).permutation(len(self.dataset))
        return [perm[k * self.batch_size:(k + 1) * self.batch_size].tolist() for k in range(len(self))]

    def _plan(self, epoch: int, idx: int):
        return self.dataset.plan(idx, PrivateStreams([self.seed & 0xFFFFFFFF, epoch, idx]))

    def _item(self, epoch: int, idx: int):
        return self.dataset.apply_plan(self._plan(epoch, idx))

    def __iter__(self):
        from concurrent.futures import ThreadPoolExecutor
        epoch, self.epoch = self.epoch, self.epoch + 1
        batches = self.batch_indices(epoch)
        with ThreadPoolExecutor(max_workers=self.num_workers, thread_name_prefix="car-reader") as pool:
            if self.device is None:
                yield from self._host_epoch(pool, epoch, batches)
            else:
                yield from self._device_epoch(pool, epoch, batches)

    def _host_epoch(self, pool, epoch, batches):
        from torch.utils.data import default_collate
        pending = []
        for k in range(len(batches) + self.prefetch):
            if k < len(batches):
                pending.append([pool.submit(self._item, epoch, i) for i in batches[k]])
            if k >= self.prefetch:
                yield default_collate([f.result() for f in pending.pop(0)])

    # ---- device path ------------------------------------------------------------------------------------------------------------
    def _device_state(self):
        if self._dev is None:
            from . import _lib
            st = {"lib": _lib.api(), "stream": torch.cuda.Stream(self.device), "slots": [], "next": 0, "scratch": None}
            with torch.cuda.device(self.device):
                st["tables"] = torch.from_numpy(frame_tables()).to(self.device)          # uploaded once
            self._dev = st
        return self._dev

    def _slot(self, st, nbytes: int):
        """The next pinned staging buffer of the ring (prefetch + 1 of them) and its device twin, grown when a batch needs more; a
        buffer is reused only after the copy that read it last has finished (its event).

        What makes the reuse safe, half by half.  The pinned half is written by the assembler thread alone, and the launchers' host-side
        validation reads the records and indices from it in that same thread right after it wrote them, so the only other reader is
        the upload copy: the slot's event, recorded behind that copy, is all a rewrite has to wait for.  The device twin needs no event:
        the next copy into it is queued on the loader's one stream, behind the two kernels that read it for the batch before."""
        if len(st["slots"]) <= st["next"]:
            st["slots"].append({"pinned": None, "dev": None, "event": None})
        slot = st["slots"][st["next"]]
        st["next"] = (st["next"] + 1) % (self.prefetch + 1)
        if slot["event"] is not None:
            slot["event"].synchronize()
        if slot["pinned"] is None or slot["pinned"].numel() < nbytes:
            slot["pinned"] = torch.empty(_align(nbytes, 1 << 20), dtype=torch.uint8).pin_memory()
        return slot

    def _prepare(self, st, plans):
        """One batch on the loader's stream: stage, upload, both launches.  Returns ((model_input, gt), event)."""
        from torch.utils.data import default_collate
        lib = st["lib"]
        frames = [f for p in plans for f in p["frames"][:p["num_query"]]] + [f for p in plans for f in p["frames"][p["num_query"]:]]
        records = [r for p in plans for r in p["records"][:p["num_query"]]] + [r for p in plans for r in p["records"][p["num_query"]:]]
        nq = sum(p["num_query"] for p in plans)
        pixels = [x for p in plans for x in p["pixels"]] + [None] * (len(frames) - nq)
        if any(r["out_hw"] != (SIDE, SIDE) for r in records):
            raise ValueError("the device path covers frames that end at 256 x 256 (stored 256 x 455 or raw 360 x 640, square_crop=True)")
        # the staging buffer: [records A | records B | indices | frames]; the device twin has the 256 x 256 windows of stage A behind it
        n_a = sum(r["resize360"] for r in records)
        n_idx = sum(len(x) for x in pixels if x is not None)
        off_a, off_b = 0, _align(n_a * FRAME_REC.itemsize)
        off_idx = off_b + _align(len(frames) * FRAME_REC.itemsize)
        at = off_idx + _align(4 * n_idx)
        frame_offs = []
        for f in frames:
            frame_offs.append(at)
            at = _align(at + f.nbytes)
        upload, total = at, at + n_a * SIDE * SIDE * 3
        recs_a, recs_b, idx = stage_records([f.shape for f in frames], records, pixels, frame_offs, upload)
        slot = self._slot(st, upload)
        host = slot["pinned"].numpy()
        host[off_a:off_a + recs_a.nbytes] = recs_a.view(np.uint8)
        host[off_b:off_b + recs_b.nbytes] = recs_b.view(np.uint8)
        host[off_idx:off_idx + idx.nbytes] = idx.view(np.uint8)
        for f, o in zip(frames, frame_offs):
            host[o:o + f.nbytes] = np.ascontiguousarray(f).reshape(-1)
        per_query = [SIDE * SIDE if x is None else len(x) for x in pixels[:nq]]
        if len(set(per_query)) != 1:
            raise ValueError("the query frames of a batch must select the same number of pixels")
        R = per_query[0]
        q_floats = int(recs_b["dst_off"][nq])                 # the context frames' outputs follow the query frames'
        with torch.cuda.device(self.device), torch.cuda.stream(st["stream"]):
            if slot["dev"] is None or slot["dev"].numel() < total:
                slot["dev"] = torch.empty(_align(total, 1 << 20), dtype=torch.uint8, device=self.device)
            dev = slot["dev"]
            dev[:upload].copy_(slot["pinned"][:upload], non_blocking=True)
            slot["event"] = torch.cuda.Event()
            slot["event"].record(st["stream"])
            n_out = int(recs_b["dst_off"][-1]) + SIDE * SIDE * 3             # the last frame is a context frame: dense
            out = torch.empty(n_out, dtype=torch.float32, device=self.device)
            base, stream = dev.data_ptr(), st["stream"].cuda_stream
            hptr = slot["pinned"].data_ptr()
            if n_a:
                lib.car_frames_resize_u8(base, upload, hptr + off_a, base + off_a, n_a, st["tables"].data_ptr(), base + upload, n_a * SIDE * SIDE * 3, stream)
            lib.car_frames_resize_f32(base, total, hptr + off_b, base + off_b, len(frames), hptr + off_idx, base + off_idx, n_idx,
                                      st["tables"].data_ptr(), out.data_ptr(), n_out, stream)
        b, Q = len(plans), plans[0]["num_query"]
        V = (len(frames) - nq) // b
        if R == SIDE * SIDE or R % 4 == 0:
            q_rgb = out[:nq * R * 3].view(b, Q, R, 3)
        else:                                                # the images' outputs are padded to 4 floats: drop the padding
            q_rgb = out[:q_floats].view(nq, -1)[:, :R * 3].reshape(b, Q, R, 3)
        c_rgb = out[q_floats:].view(b, V, SIDE, SIDE, 3)
        cams = default_collate([{"query": p["query"], "context": p["context"]} for p in plans])
        place = (lambda t: t) if self.cameras == "host" else (lambda t: t.to(self.device, non_blocking=True))
        with torch.cuda.device(self.device), torch.cuda.stream(st["stream"]):
            query = {"rgb": q_rgb, "cam2world": place(cams["query"]["cam2world"]), "intrinsics": place(cams["query"]["intrinsics"]),
                     "uv": cams["query"]["uv"].to(self.device, non_blocking=True), "mask": cams["query"]["mask"].to(self.device, non_blocking=True)}
            context = {"rgb": c_rgb, "cam2world": place(cams["context"]["cam2world"]), "intrinsics": place(cams["context"]["intrinsics"])}
            done = torch.cuda.Event()
            done.record(st["stream"])
        return ({"query": query, "context": context}, query), done

    def _device_epoch(self, pool, epoch, batches):
        import queue
        import threading
        st = self._device_state()
        ready, stop = queue.Queue(maxsize=self.prefetch), threading.Event()

        def put(x):
            while not stop.is_set():
                try:
                    ready.put(x, timeout=0.1)
                    return
                except queue.Full:
                    pass

        def assemble():
            try:
                pending = []
                for k in range(len(batches) + self.prefetch):
                    if stop.is_set():
                        return
                    if k < len(batches):
                        pending.append([pool.submit(self._plan, epoch, i) for i in batches[k]])
                    if k >= self.prefetch:
                        put(self._prepare(st, [f.result() for f in pending.pop(0)]))
                put(None)
            except BaseException as e:                       # handed to the consumer, which raises it
                put(e)

        worker = threading.Thread(target=assemble, name="car-assembler", daemon=True)
        worker.start()
        try:
            while True:
                got = ready.get()
                if got is None:
                    return
                if isinstance(got, BaseException):
                    raise got
                batch, done = got
                cur = torch.cuda.current_stream(self.device)
                cur.wait_event(done)
                for part in batch[0].values():               # the tensors were allocated on the loader's stream and are used on this one
                    for t in part.values():
                        if torch.is_tensor(t) and t.is_cuda:
                            t.record_stream(cur)
                yield batch
        finally:
            stop.set()
            worker.join()
