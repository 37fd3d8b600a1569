"""Render / eval plumbing shared by ``experiment_scripts/`` (reference render_realestate10k_traj.py:84-183,
eval_realestate10k.py:123-199): chunked rendering of a frame, trajectory construction, PSNR, frame output.

Everything numerically interesting happens inside ``CrossAttentionRenderer.forward``; this module only slices rays
into chunks, shards them over ranks and puts the tiles back together.
"""
from __future__ import annotations

import ctypes
import math
import os
import zlib
import struct
from typing import Dict, List, Optional

import torch

from . import _lib, sharding, synthetic

CHUNK_RAYS = 8192          # render_realestate10k_traj.py:96


CAMERA_KEYS = ("cam2world", "intrinsics")


def to_device(inp, device, cameras: str = "host"):
    """Moves an input dict to the device.  All three choices but the last give the strict-parity pose algebra (the reference's own
    ``torch.inverse`` / ``matmul`` on the host CPU, poses.pack_poses; the reference's fixtures reproduce to 1e-4):
      ``"host"`` (default) leaves the 4x4 camera matrices on the CPU — the engine uploads 768 bytes of records per new pose and never
                 waits for the device;
      ``"gpu"``  moves them too, as the reference's ``dict_to_gpu`` does (render_realestate10k_traj.py:85): the engine copies them back
                 for the host algebra, one small download + stream synchronisation per new pose (engine._poses);
      ``"device"`` moves them and is meant for a module with ``pose_route = "device"``: ``car_pose_setup`` on the GPU, no host work per
                 frame, equal to the host algebra to a few ulp — which the fp64 Pluecker intersection amplifies on near-parallel
                 samples."""
    if cameras not in ("host", "gpu", "device"):
        raise ValueError("cameras must be 'host', 'gpu' or 'device'")
    keep = CAMERA_KEYS if cameras == "host" else ()
    return {k: {kk: (vv.to(device) if torch.is_tensor(vv) and kk not in keep else vv) for kk, vv in v.items()} for k, v in inp.items()}


@torch.no_grad()
def render_frame(model, model_input, z, chunk_rays: int = CHUNK_RAYS, rank: int = 0, world: int = 1) -> torch.Tensor:
    """Renders every query ray of ``model_input`` in chunks (the reference's loop, render_realestate10k_traj.py:118-145).
    With world > 1 this rank renders its ray band and the tiles are all-gathered.  Returns (b, R, 5) = rgb, depth, valid."""
    n_rays = model_input["query"]["uv"].shape[2]
    shard, (s, e) = sharding.shard_query(model_input, rank, world) if world > 1 else (model_input, (0, n_rays))
    uv = shard["query"]["uv"]
    tiles = []
    for c0 in range(0, uv.shape[2], chunk_rays):
        chunk = {"context": shard["context"], "query": dict(shard["query"], uv=uv[:, :, c0:c0 + chunk_rays])}
        tiles.append(sharding.pack_tile(model(chunk, z=z)))
    tile = torch.cat(tiles, dim=1)
    return sharding.gather_rays(tile, n_rays) if world > 1 else tile


def trajectory(inp, n_frames: int) -> List[Dict]:
    """One input dict per frame of a camera path between the first and the last context camera of every scene:
    ``trajectory.linear_interpolate`` (the reference's load_video_superglue.linear_interpolate: rotation by slerp, position on the
    segment), ``n_frames`` poses including both ends."""
    from . import trajectory as T
    c2w = inp["context"]["cam2world"]
    b = c2w.shape[0]
    paths = [T.linear_interpolate(c2w[s, [0, -1]].double().cpu().numpy(), max(n_frames, 2)) for s in range(b)]
    frames = []
    for i in range(n_frames):
        q = torch.stack([torch.from_numpy(paths[s][i]).float() for s in range(b)])[:, None]
        frames.append({"context": inp["context"], "query": dict(inp["query"], cam2world=q.to(inp["query"]["cam2world"].device))})
    return frames


def psnr(img: torch.Tensor, ref: torch.Tensor) -> float:
    """mse2psnr of the reference scripts (render_realestate10k_traj.py:34-35), images in [0, 1]."""
    mse = torch.mean((img - ref) ** 2).item()
    return float("inf") if mse == 0 else -10.0 * math.log10(mse)


def ssim(img: torch.Tensor, ref: torch.Tensor, data_range: float = 2.0) -> torch.Tensor:
    """SSIM of the reference's eval script (eval_realestate10k.py:192-194: scikit-image 0.18.3 ``structural_similarity(x, y,
    win_size=11, multichannel=True, gaussian_weights=True)``) on the device: ``car_ssim`` (csrc/car_metrics.hip).

    ``img`` and ``ref`` are (H, W, C) or (B, H, W, C) tensors on a ROCm device, C in 1..4, H and W >= 11; they are taken as
    contiguous float32.  Returns a float64 device tensor of shape () or (B,), each pair's mean over channels of the mean SSIM
    over the pixels at least 5 from every edge.  The launch goes on the current stream and nothing waits for it: ``.item()``
    synchronises.

    ``data_range`` defaults to 2.0, not 1.0, on purpose: the reference passes none, and scikit-image 0.18.3 then takes the range
    of its float dtype, -1..1, so the paper's SSIM figures use C1 = 0.02**2 and C2 = 0.06**2 even for images in [0, 1].  Pass 1.0
    for the usual convention for [0, 1] images.

    Raises ValueError for CPU tensors (there is no CPU fallback), mismatched shapes and the shapes / ranges car_ssim refuses."""
    if not (torch.is_tensor(img) and torch.is_tensor(ref)):
        raise ValueError("ssim: img and ref must be tensors")
    if img.device.type != "cuda" or ref.device != img.device:
        raise ValueError(f"ssim: needs both images on one ROCm device (got {img.device} and {ref.device}); there is no CPU fallback")
    if img.shape != ref.shape or img.dim() not in (3, 4):
        raise ValueError(f"ssim: need two (H, W, C) or (B, H, W, C) images of one shape, got {tuple(img.shape)} and {tuple(ref.shape)}")
    x, y = (t.to(torch.float32).contiguous() for t in (img, ref))
    B, H, W, C = x.shape if x.dim() == 4 else (1, *x.shape)
    lib = _lib.api()
    with torch.cuda.device(x.device):
        n = lib.car_ssim_scratch_doubles(B, H, W, C)
        out = torch.empty(B, dtype=torch.float64, device=x.device)
        scratch = torch.empty(max(n, 1), dtype=torch.float64, device=x.device)      # car_ssim refuses the shape when n == 0
        _lib.user_call(lib.car_ssim, x.data_ptr(), y.data_ptr(), B, H, W, C, ctypes.c_double(data_range), out.data_ptr(), scratch.data_ptr(), n, _lib.stream())
    return out[0] if img.dim() == 3 else out


# ---- LPIPS v0.1, net = 'vgg' (car_lpips, csrc/car_lpips.hip) ---------------------------------------------------------
LPIPS_FEATURES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)      # torchvision vgg16().features indices of the 13 convolutions
LPIPS_WIDTHS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
LPIPS_SLICE = (1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5)                   # the lpips package's net.slice{n} that holds each of them
LPIPS_TAP_WIDTHS = (64, 128, 256, 512, 512)
LPIPS_SHIFT = (-0.030, -0.088, -0.188)
LPIPS_SCALE = (0.458, 0.448, 0.450)


def lpips_arrays(vgg_state, lin_state=None):
    """The 13 convolutions' weights and biases and the five ``lin`` weights as float32 CPU tensors, from either layout of weight files:
    a torchvision VGG16 state dict (``features.{i}.weight|bias``) plus the lpips package's linear file (``lin{k}.model.1.weight``), or
    — with ``lin_state`` None — one ``lpips.LPIPS(net='vgg').state_dict()`` (``net.slice{n}.{i}.weight|bias``, ``lin{k}.model.1.weight``;
    its duplicate ``lins.*`` keys are ignored, its ``scaling_layer.shift|scale`` checked against the constants).
    Raises ValueError naming the key that is missing or has the wrong shape.  The sign of a lin weight is not checked."""
    def take(state, key, shape):
        if key not in state:
            raise ValueError(f"lpips weights: key {key!r} is missing")
        t = state[key]
        if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape):
            raise ValueError(f"lpips weights: key {key!r} has shape {tuple(getattr(t, 'shape', ()))}, need {tuple(shape)}")
        return t.detach().to("cpu", torch.float32).contiguous()
    single = lin_state is None
    lin_state = vgg_state if single else lin_state
    conv_w, conv_b, k_in = [], [], 3
    for i, n, sl in zip(LPIPS_FEATURES, LPIPS_WIDTHS, LPIPS_SLICE):
        stem = f"net.slice{sl}.{i}" if single else f"features.{i}"
        conv_w.append(take(vgg_state, stem + ".weight", (n, k_in, 3, 3)))
        conv_b.append(take(vgg_state, stem + ".bias", (n,)))
        k_in = n
    lin = [take(lin_state, f"lin{k}.model.1.weight", (1, c, 1, 1)).reshape(c) for k, c in enumerate(LPIPS_TAP_WIDTHS)]
    if single:
        for key, want in (("scaling_layer.shift", LPIPS_SHIFT), ("scaling_layer.scale", LPIPS_SCALE)):
            if key in vgg_state:
                got = vgg_state[key]
                if not torch.is_tensor(got) or got.numel() != 3 or (got.double().reshape(3) - torch.tensor(want, dtype=torch.float64)).abs().max() > 1e-6:
                    raise ValueError(f"lpips weights: key {key!r} differs from LPIPS v0.1's constants {want}")
    return conv_w, conv_b, lin


class LpipsWeights:
    """The caller's LPIPS weights: the float32 arrays, and per device their packed form (car_lpips_pack, made once) and the
    workspaces of the shapes evaluated so far."""

    def __init__(self, conv_w, conv_b, lin):
        self.conv_w, self.conv_b, self.lin = conv_w, conv_b, lin
        self._packed, self._packed_backward, self._work = {}, {}, {}

    def _pack_once(self, cache, device, groups, floats, pack) -> torch.Tensor:
        """``cache[device]``, made on first use: the float32 tensor lists ``groups`` go to the device, entry ``pack`` (one table of
        pointers per group, the output, the stream) writes entry ``floats``'s count of floats.  The one key rule of both packed forms."""
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"lpips: the weights are packed on a ROCm device, not on {device}; there is no CPU fallback")
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        if key not in cache:
            lib = _lib.api()
            with torch.cuda.device(device):
                dev = [[t.to(device) for t in group] for group in groups]
                tables = [(ctypes.c_void_p * len(g))(*[t.data_ptr() for t in g]) for g in dev]
                out = torch.empty(getattr(lib, floats)(), dtype=torch.float32, device=device)
                getattr(lib, pack)(*tables, out.data_ptr(), _lib.stream())
                torch.cuda.current_stream().synchronize()              # the float32 copies in `dev` are released on return
            cache[key] = out
        return cache[key]

    def packed(self, device) -> torch.Tensor:
        return self._pack_once(self._packed, device, (self.conv_w, self.conv_b, self.lin), "car_lpips_packed_floats", "car_lpips_pack")

    def packed_backward(self, device) -> torch.Tensor:
        """The data gradients' weights (car_lpips_pack_backward: every layer but the first, transposed and flipped), made on the first
        backward on a device."""
        return self._pack_once(self._packed_backward, device, (self.conv_w,), "car_lpips_backward_packed_floats", "car_lpips_pack_backward")

    def workspace(self, device, B, H, W, nbytes) -> torch.Tensor:
        key = (str(device), B, H, W)
        if key not in self._work:
            self._work[key] = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
        return self._work[key]


def load_lpips_weights(vgg_path: str, lin_path: Optional[str] = None) -> LpipsWeights:
    """Reads the LPIPS weight files the caller names (``torch.load(..., weights_only=True)``): a torchvision VGG16 state dict and the
    lpips package's ``vgg.pth``, or one file holding ``lpips.LPIPS(net='vgg').state_dict()``.  Validates every key (``lpips_arrays``);
    packing happens once per device, on first use."""
    vgg = torch.load(vgg_path, map_location="cpu", weights_only=True)
    lin = torch.load(lin_path, map_location="cpu", weights_only=True) if lin_path else None
    return LpipsWeights(*lpips_arrays(vgg, lin))


def lpips(img: torch.Tensor, ref: torch.Tensor, weights: LpipsWeights, return_taps: bool = False):
    """LPIPS v0.1 (net = 'vgg') of the reference's eval script (eval_realestate10k.py:184-191: ``loss_fn_vgg((x - 0.5) * 2, (y - 0.5) * 2)``)
    on the device: ``car_lpips`` (csrc/car_lpips.hip) with the caller's weights (``load_lpips_weights``).

    ``img`` and ``ref`` are (H, W, 3) or (B, H, W, 3) tensors in [0, 1] on a ROCm device, H and W >= 16; they are mapped to [-1, 1]
    here, as the reference does.  Returns a float64 device tensor of shape () or (B,) (with ``return_taps`` also the five per-tap
    terms, (5,) or (B, 5)).  Nothing waits for the launches.  Identical images give exactly 0.

    Raises ValueError for CPU tensors (there is no CPU fallback), mismatched shapes and the shapes car_lpips refuses."""
    if not (torch.is_tensor(img) and torch.is_tensor(ref)):
        raise ValueError("lpips: img and ref must be tensors")
    if img.device.type != "cuda" or ref.device != img.device:
        raise ValueError(f"lpips: needs both images on one ROCm device (got {img.device} and {ref.device}); there is no CPU fallback")
    if img.shape != ref.shape or img.dim() not in (3, 4) or img.shape[-1] != 3:
        raise ValueError(f"lpips: need two (H, W, 3) or (B, H, W, 3) images of one shape, got {tuple(img.shape)} and {tuple(ref.shape)}")
    if not isinstance(weights, LpipsWeights):
        raise ValueError("lpips: weights must come from load_lpips_weights")
    x, y = (((t.to(torch.float32) - 0.5) * 2).contiguous() for t in (img, ref))
    B, H, W, _ = x.shape if x.dim() == 4 else (1, *x.shape)
    lib = _lib.api()
    with torch.cuda.device(x.device):
        packed = weights.packed(x.device)
        n = lib.car_lpips_workspace_bytes(B, H, W)
        work = weights.workspace(x.device, B, H, W, n)
        out = torch.empty(max(B, 1), dtype=torch.float64, device=x.device)
        taps = torch.empty(max(B, 1), 5, dtype=torch.float64, device=x.device)
        _lib.user_call(lib.car_lpips, x.data_ptr(), y.data_ptr(), B, H, W, packed.data_ptr(), out.data_ptr(), taps.data_ptr(), work.data_ptr(), n, _lib.stream())
    out, taps = (out[0], taps[0]) if img.dim() == 3 else (out, taps)
    return (out, taps) if return_taps else out


class _LpipsLoss(torch.autograd.Function):
    """car_lpips_forward_train / car_lpips_backward.  The workspace with the 13 retained activation maps belongs to the call (two losses
    may be alive before either runs backward), so it is allocated here, not cached on the weights."""

    @staticmethod
    def forward(ctx, x, y, weights):
        lib = _lib.api()
        xc, yc = x.detach().contiguous(), y.detach().contiguous()
        B, H, W, _ = xc.shape
        with torch.cuda.device(xc.device):
            packed = weights.packed(xc.device)
            n = lib.car_lpips_train_workspace_bytes(B, H, W)
            work = torch.empty(max(n, 16), dtype=torch.uint8, device=xc.device)
            out = torch.empty(max(B, 1), dtype=torch.float64, device=xc.device)
            _lib.user_call(lib.car_lpips_forward_train, xc.data_ptr(), yc.data_ptr(), B, H, W, packed.data_ptr(), out.data_ptr(), None, work.data_ptr(), n,
                           _lib.stream())
        ctx.weights, ctx.work, ctx.shape = weights, work, (B, H, W)
        return out

    @staticmethod
    def backward(ctx, g):
        B, H, W = ctx.shape
        need_x, need_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_x or need_y):
            return None, None, None
        dev = ctx.work.device
        g = g.to(torch.float64).contiguous()
        with torch.cuda.device(dev):
            gx = torch.empty(B, H, W, 3, dtype=torch.float32, device=dev) if need_x else None
            gy = torch.empty(B, H, W, 3, dtype=torch.float32, device=dev) if need_y else None
            _lib.api().car_lpips_backward(g.data_ptr(), gx.data_ptr() if need_x else None, gy.data_ptr() if need_y else None, B, H, W,
                                          ctx.weights.packed(dev).data_ptr(), ctx.weights.packed_backward(dev).data_ptr(), ctx.work.data_ptr(),
                                          ctx.work.numel(), _lib.stream())
        return gx, gy, None


def lpips_loss(x: torch.Tensor, y: torch.Tensor, weights: LpipsWeights) -> torch.Tensor:
    """LPIPS v0.1 (net = 'vgg') as a training loss, the reference's ``LFLoss(lpips=True)`` term (loss_functions.py:102-118:
    ``loss_fn_vgg(gt_rgb, pred_rgb)`` on the model's own rgb range): ``car_lpips_forward_train`` and, under autograd,
    ``car_lpips_backward`` (csrc/car_lpips.hip).  The network's weights are frozen.

    ``x`` and ``y`` are (B, H, W, 3) float32 tensors in [-1, 1] on one ROCm device, H and W >= 16; unlike ``lpips`` nothing is remapped.
    Returns a float64 (B,) tensor, the same bits ``lpips`` gives for the same [-1, 1] images; its backward gives float32 gradients to
    whichever of ``x``, ``y`` requires one and walks only that image stack.  Bit-reproducible; nothing waits for the launches.

    Raises ValueError for CPU tensors (there is no CPU fallback), mismatched shapes and the shapes car_lpips refuses."""
    if not (torch.is_tensor(x) and torch.is_tensor(y)):
        raise ValueError("lpips_loss: x and y must be tensors")
    if x.device.type != "cuda" or y.device != x.device:
        raise ValueError(f"lpips_loss: needs both images on one ROCm device (got {x.device} and {y.device}); there is no CPU fallback")
    if x.shape != y.shape or x.dim() != 4 or x.shape[-1] != 3:
        raise ValueError(f"lpips_loss: need two (B, H, W, 3) images of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.dtype != torch.float32 or y.dtype != torch.float32:
        raise ValueError(f"lpips_loss: need float32 images, got {x.dtype} and {y.dtype}")
    if not isinstance(weights, LpipsWeights):
        raise ValueError("lpips_loss: weights must come from load_lpips_weights")
    return _LpipsLoss.apply(x, y, weights)


# ---- relative pose of an unposed pair (car_essential_ransac, csrc/car_pose.hip) -----------------------------------------
def pose_sample_table(n: int, hypotheses: int, seed: int = 0):
    """The five-point sample table: ``hypotheses`` rows of five distinct indices below ``n`` as int32, uniform over ordered 5-tuples,
    from ``numpy.random.default_rng(seed)`` (one ``integers`` call; the k-th index of a row is drawn among the n - k values its row
    has not taken yet)."""
    import numpy as np
    g = np.random.default_rng(seed)
    draws = g.integers(0, np.array([n, n - 1, n - 2, n - 3, n - 4]), size=(hypotheses, 5))
    out = np.empty((hypotheses, 5), dtype=np.int64)
    for k in range(5):
        idx = draws[:, k].copy()
        prev = np.sort(out[:, :k], axis=1)
        for j in range(k):
            idx += idx >= prev[:, j]
        out[:, k] = idx
    return out.astype(np.int32)


def recover_pose(E, x0, x1, mask, dist: float = 1e9):
    """OpenCV's ``recoverPose`` written down from its documented procedure, in float64 on the host (a few KB once per pair).  SVD of E
    with U and V^T sign-fixed to determinant +1; R1 = U W V^T, R2 = U W^T V^T, t = U[:, 2]; the combinations (R1, t), (R2, t),
    (R1, -t), (R2, -t) in this order; for each the matches of ``mask`` are triangulated linearly with P0 = [I | 0], P1 = [R | t] and
    those with 0 < z < ``dist`` in both cameras counted; the first combination with the largest count wins.  Returns (count, R, t,
    mask of the matches that passed for the winner).  Not pinned against cv2, which is not available offline."""
    import numpy as np
    E = np.asarray(E, dtype=np.float64).reshape(3, 3)
    U, _, Vt = np.linalg.svd(E)
    U = -U if np.linalg.det(U) < 0 else U
    Vt = -Vt if np.linalg.det(Vt) < 0 else Vt
    W = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    R1, R2, t = U @ W @ Vt, U @ W.T @ Vt, U[:, 2]
    mask = np.asarray(mask).astype(bool)
    sel = np.nonzero(mask)[0]
    a, b = np.asarray(x0, dtype=np.float64)[sel], np.asarray(x1, dtype=np.float64)[sel]
    best = None
    for R, tt in ((R1, t), (R2, t), (R1, -t), (R2, -t)):
        P1 = np.concatenate([R, tt[:, None]], axis=1)
        A = np.zeros((len(sel), 4, 4))                                  # x (P row 3) - (P row 1), y (P row 3) - (P row 2), both views
        A[:, 0, 0], A[:, 0, 2] = -1.0, a[:, 0]
        A[:, 1, 1], A[:, 1, 2] = -1.0, a[:, 1]
        A[:, 2] = b[:, 0, None] * P1[2][None] - P1[0][None]
        A[:, 3] = b[:, 1, None] * P1[2][None] - P1[1][None]
        Q = np.linalg.svd(A)[2][:, 3] if len(sel) else np.zeros((0, 4))
        with np.errstate(all="ignore"):
            X = Q[:, :3] / Q[:, 3:4]
            z0, z1 = X[:, 2], (X @ R.T + tt)[:, 2]
            good = (z0 > 0) & (z0 < dist) & (z1 > 0) & (z1 < dist)
        if best is None or int(good.sum()) > best[0]:
            best = (int(good.sum()), R, tt, good)
    out = np.zeros(mask.shape[0], dtype=bool)
    out[sel] = best[3]
    return best[0], best[1], best[2], out


def estimate_pose(kpts0, kpts1, K0, K1, thresh, hypotheses: int = 8192, seed: int = 0, device=None):
    """Relative pose of the second view from keypoint matches, the reference's ``estimate_pose`` (dataset/load_video_superglue.py:
    114-138) with its signature and conventions: ``kpts0``, ``kpts1`` (N, 2) matched pixels, ``K0``, ``K1`` intrinsics, ``thresh`` in
    pixels; ``norm_thresh = thresh / mean(K0[0,0], K1[1,1], K0[0,0], K1[1,1])``, points normalised with ``K[[0,1],[2,2]]`` and
    ``K[[0,1],[0,1]]``.  Returns ``(R, t, inlier_mask)`` with x_2 = R x_1 + t, |t| = 1 and the mask as cv2 leaves it after recoverPose
    (the winner's inliers that triangulate in front of both cameras), or None below five matches or when no hypothesis gives a pose.

    The essential matrix comes from ``car_essential_ransac`` on the device (csrc/car_pose.hip), all fp64.  In place of cv2's
    ``prob=0.99999`` stop rule (at most 1000 iterations) there is a FIXED BUDGET: ``hypotheses`` five-point samples, drawn on the host
    from ``numpy.random.default_rng(seed)`` (``pose_sample_table``), uploaded once, every one solved and scored against every match.
    Scoring a superset of hypotheses can never return fewer inliers, so a larger budget only helps; the result is a function of the
    inputs, ``hypotheses`` and ``seed`` alone (ties: lowest hypothesis, then lowest candidate).  The default of 8192 is no measured
    optimum: at 30-40 % inliers 300 hypotheses are too few and 4000 are enough (profiles/pose_estimate.md).  recoverPose runs on the
    host in float64 (``recover_pose``).  Neither stage is pinned against cv2.

    Raises ValueError for shapes the device entry refuses, RuntimeError without a ROCm device (there is no CPU fallback)."""
    import numpy as np
    kpts0, kpts1 = np.asarray(kpts0, dtype=np.float64), np.asarray(kpts1, dtype=np.float64)
    if kpts0.ndim != 2 or kpts0.shape[1] != 2 or kpts0.shape != kpts1.shape:
        raise ValueError(f"estimate_pose: need two (N, 2) arrays of matched keypoints, got {kpts0.shape} and {kpts1.shape}")
    if len(kpts0) < 5:
        return None
    K0, K1 = np.asarray(K0, dtype=np.float64), np.asarray(K1, dtype=np.float64)
    f_mean = np.mean([K0[0, 0], K1[1, 1], K0[0, 0], K1[1, 1]])
    norm_thresh = float(thresh / f_mean)
    x0 = np.ascontiguousarray((kpts0 - K0[[0, 1], [2, 2]][None]) / K0[[0, 1], [0, 1]][None])
    x1 = np.ascontiguousarray((kpts1 - K1[[0, 1], [2, 2]][None]) / K1[[0, 1], [0, 1]][None])
    if not torch.cuda.is_available():
        raise RuntimeError("estimate_pose: needs a ROCm device; there is no CPU fallback")
    dev = torch.device(device if device is not None else "cuda")
    N, H = len(x0), int(hypotheses)
    lib = _lib.api()
    nbytes = lib.car_essential_workspace_bytes(N, H)
    if nbytes == 0:                                         # the size entry's refusal: CAR_E_ARG, with its message
        _lib.user_call(_lib.check, _lib.CAR_E_ARG, "car_essential_workspace_bytes")
    with torch.cuda.device(dev):
        d0, d1 = torch.from_numpy(x0).to(dev), torch.from_numpy(x1).to(dev)
        table = torch.from_numpy(pose_sample_table(N, H, seed)).to(dev)
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        E = torch.empty(9, dtype=torch.float64, device=dev)
        best = torch.empty(3, dtype=torch.int32, device=dev)
        inl = torch.empty(N, dtype=torch.uint8, device=dev)
        _lib.user_call(lib.car_essential_ransac, d0.data_ptr(), d1.data_ptr(), N, table.data_ptr(), H, ctypes.c_double(norm_thresh), E.data_ptr(),
                       best.data_ptr(), inl.data_ptr(), work.data_ptr(), nbytes, _lib.stream())
        E, best, inl = E.cpu().numpy(), best.cpu().numpy(), inl.cpu().numpy()
    if best[0] < 1:
        return None
    n, R, t, mask = recover_pose(E, x0, x1, inl)
    return (R, t, mask) if n > 0 else None


def write_png(path: str, rgb: torch.Tensor) -> None:
    """(H, W, 3) float image in [-1, 1] -> 8-bit PNG (imageio is not available in this image)."""
    img = ((rgb.clamp(-1, 1) + 1) * 127.5).round().to(torch.uint8).cpu().numpy()
    h, w, _ = img.shape
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


_JET_SEGMENTS = (((0.00, 0, 0), (0.35, 0, 0), (0.66, 1, 1), (0.89, 1, 1), (1.00, 0.5, 0.5)),                          # red
                 ((0.000, 0, 0), (0.125, 0, 0), (0.375, 1, 1), (0.640, 1, 1), (0.910, 0, 0), (1.000, 0, 0)),        # green
                 ((0.00, 0.5, 0.5), (0.11, 1, 1), (0.34, 1, 1), (0.65, 0, 0), (1.00, 0, 0)))                       # blue
_jet_lut = None


def jet_lut() -> torch.Tensor:
    """The 256-entry "jet" table as a (256, 3) float32 CPU tensor, for ``car_colormap`` (summaries.colormap): matplotlib's lookup-table
    construction restated — each channel's piecewise-linear segments (x, y below, y above) sampled at ``linspace(0, 1, 256)`` in
    float64, the first and last entries taken from the end segments, clipped to [0, 1] — then cast to float32.  Equal to
    ``matplotlib.pyplot.get_cmap("jet")``'s table entry for entry after the cast (tests/test_summaries_cpu.py)."""
    global _jet_lut
    if _jet_lut is None:
        import numpy as np
        n, cols = 256, []
        for segments in _JET_SEGMENTS:
            seg = np.array(segments, dtype=np.float64)
            x, below, above = seg[:, 0] * (n - 1), seg[:, 1], seg[:, 2]
            at = (n - 1) * np.linspace(0, 1, n)
            hi = np.searchsorted(x, at)[1:-1]
            frac = (at[1:-1] - x[hi - 1]) / (x[hi] - x[hi - 1])
            cols.append(np.clip(np.concatenate([[above[0]], frac * (below[hi] - above[hi - 1]) + above[hi - 1], [below[-1]]]), 0.0, 1.0))
        _jet_lut = torch.from_numpy(np.stack(cols, axis=-1).astype(np.float32))
    return _jet_lut


def synthetic_pair(H: int, n_view: int, seed: int = 5):
    """A seeded stereo pair + feature pyramid standing in for a dataset item and ``get_z`` (no dataset / encoder here)."""
    inp = synthetic.stereo_scene(H, b=1, seed=seed, n_view=n_view)
    z = synthetic.feature_maps(1, n_view, H, seed=1)
    return inp, z
