"""Matching an unposed pair on the device: SuperPoint's and SuperGlue's forwards (the reference's estimate_pose/superpoint.py,
superglue.py, glue_match.py) through ``csrc/car_superpoint.hip`` and ``csrc/car_superglue.hip``.  The weights are
the caller's; none are shipped.  There is no CPU fallback."""
from __future__ import annotations

import ctypes
from typing import Dict, List, Mapping, Optional, Sequence

import torch

from . import _lib

# the reference module's convolutions in declaration order: name, input channels, output channels, kernel size
SUPERPOINT_CONVS = (("conv1a", 1, 64, 3), ("conv1b", 64, 64, 3), ("conv2a", 64, 64, 3), ("conv2b", 64, 64, 3), ("conv3a", 64, 128, 3),
                    ("conv3b", 128, 128, 3), ("conv4a", 128, 128, 3), ("conv4b", 128, 128, 3), ("convPa", 128, 256, 3), ("convPb", 256, 65, 1),
                    ("convDa", 128, 256, 3), ("convDb", 256, 256, 1))
MAX_KEYPOINTS = 4096


def superpoint_arrays(state: Mapping[str, torch.Tensor]):
    """The twelve convolutions of a SuperPoint state dict (the reference module's parameter names) as float32 CPU tensors, in
    declaration order.  A missing or mis-shaped key is a ValueError that names it."""
    conv_w, conv_b = [], []
    for name, k, n, ks in SUPERPOINT_CONVS:
        for key, shape, into in ((f"{name}.weight", (n, k, ks, ks), conv_w), (f"{name}.bias", (n,), conv_b)):
            if key not in state:
                raise ValueError(f"superpoint weights: key {key!r} is missing")
            t = state[key]
            if not torch.is_tensor(t) or tuple(t.shape) != shape:
                raise ValueError(f"superpoint weights: key {key!r} has shape {tuple(getattr(t, 'shape', ()))}, expected {shape}")
            into.append(t.detach().to("cpu", torch.float32).contiguous())
    return conv_w, conv_b


KENC_WIDTHS = (3, 32, 64, 128, 256, 256)
KENC_CONVS = (0, 3, 6, 9, 12)                          # kenc.encoder's convolutions; a BatchNorm1d behind each of the first four
MAX_GLUE_KEYPOINTS = 1024
_BN = ("weight", "bias", "running_mean", "running_var")


def superglue_arrays(state: Mapping[str, torch.Tensor], gnn_layers: Optional[Sequence[str]] = None):
    """A SuperGlue state dict (the reference module's parameter names) as car_superglue_pack's list of float32 CPU tensors, the layers'
    ``self`` / ``cross`` pattern and bin_score.  ``gnn_layers`` defaults to the reference's alternation over the layers the dict holds.
    A missing or mis-shaped key is a ValueError that names it."""
    n_layers = 1 + max([int(k.split(".")[2]) for k in state if k.startswith("gnn.layers.")], default=-1)
    if gnn_layers is None:
        gnn_layers = ["self", "cross"] * (n_layers // 2) + ["self"] * (n_layers % 2)
    gnn_layers = list(gnn_layers)
    if not gnn_layers:
        raise ValueError("superglue weights: zero GNN layers (no 'gnn.layers.*' key)")
    if any(n not in ("self", "cross") for n in gnn_layers):
        raise ValueError(f"superglue weights: GNN layer names must be 'self' or 'cross', got {gnn_layers}")
    out = []

    def take(key, shape):
        if key not in state:
            raise ValueError(f"superglue weights: key {key!r} is missing")
        t = state[key]
        if not torch.is_tensor(t) or tuple(t.shape) != shape:
            raise ValueError(f"superglue weights: key {key!r} has shape {tuple(getattr(t, 'shape', ()))}, expected {shape}")
        return t.detach().to("cpu", torch.float32).contiguous()

    def conv(name, k, n, bn=None):
        out.extend([take(name + ".weight", (n, k, 1)), take(name + ".bias", (n,))])
        if bn:
            out.extend(take(f"{bn}.{part}", (n,)) for part in _BN)
    for i, idx in enumerate(KENC_CONVS):
        conv(f"kenc.encoder.{idx}", KENC_WIDTHS[i], KENC_WIDTHS[i + 1], f"kenc.encoder.{idx + 1}" if i < 4 else None)
    for l in range(len(gnn_layers)):
        pre = f"gnn.layers.{l}"
        for j in range(3):
            conv(f"{pre}.attn.proj.{j}", 256, 256)
        conv(f"{pre}.attn.merge", 256, 256)
        conv(f"{pre}.mlp.0", 512, 512, f"{pre}.mlp.1")
        conv(f"{pre}.mlp.3", 512, 256)
    conv("final_proj", 256, 256)
    return out, gnn_layers, float(take("bin_score", ()))


class MatcherWeights:
    """The caller's matcher weights: the float32 arrays and, per device, their packed forms (car_superpoint_pack, car_superglue_pack,
    each made once, on first use).  Without a SuperGlue state dict only ``superpoint`` is served."""

    def __init__(self, superpoint_state: Mapping[str, torch.Tensor], superglue_state: Optional[Mapping[str, torch.Tensor]] = None,
                 gnn_layers: Optional[Sequence[str]] = None):
        self.conv_w, self.conv_b = superpoint_arrays(superpoint_state)
        self._packed: Dict[tuple, torch.Tensor] = {}
        self.glue = None
        if superglue_state is not None:
            self.glue, self.gnn_layers, self.bin_score = superglue_arrays(superglue_state, gnn_layers)
        self._packed_glue: Dict[tuple, torch.Tensor] = {}

    def packed_glue(self, device) -> torch.Tensor:
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"superglue: the weights are packed on a ROCm device, not on {device}; there is no CPU fallback")
        if self.glue is None:
            raise ValueError("superglue: these weights hold no SuperGlue state dict (load_matcher_weights(superpoint_path, superglue_path))")
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        if key not in self._packed_glue:
            lib, layers = _lib.api(), len(self.gnn_layers)
            with torch.cuda.device(device):
                dev = [t.to(device) for t in self.glue]
                table = (ctypes.c_void_p * len(dev))(*[t.data_ptr() for t in dev])
                out = torch.empty(lib.car_superglue_packed_floats(layers), dtype=torch.float32, device=device)
                lib.car_superglue_pack(table, len(dev), layers, out.data_ptr(), _lib.stream())
                torch.cuda.current_stream().synchronize()              # the float32 copies in `dev` are released on return
            self._packed_glue[key] = out
        return self._packed_glue[key]

    def packed(self, device) -> torch.Tensor:
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"superpoint: the weights are packed on a ROCm device, not on {device}; there is no CPU fallback")
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        if key not in self._packed:
            lib = _lib.api()
            with torch.cuda.device(device):
                dev = [[t.to(device) for t in group] for group in (self.conv_w, self.conv_b)]
                tables = [(ctypes.c_void_p * len(g))(*[t.data_ptr() for t in g]) for g in dev]
                out = torch.empty(lib.car_superpoint_packed_floats(), dtype=torch.float32, device=device)
                lib.car_superpoint_pack(*tables, out.data_ptr(), _lib.stream())
                torch.cuda.current_stream().synchronize()              # the float32 copies in `dev` are released on return
            self._packed[key] = out
        return self._packed[key]


def load_matcher_weights(superpoint_path: str, superglue_path: Optional[str] = None, gnn_layers: Optional[Sequence[str]] = None) -> MatcherWeights:
    """Reads the weight files the caller names (``torch.load(..., weights_only=True)``; the published ``superpoint_v1.pth`` and
    ``superglue_indoor.pth`` hold the reference modules' state dicts) and validates every key; packing happens once per device, on
    first use."""
    load = lambda path: torch.load(path, map_location="cpu", weights_only=True)
    return MatcherWeights(load(superpoint_path), load(superglue_path) if superglue_path else None, gnn_layers)


def superpoint(gray: torch.Tensor, weights: MatcherWeights, nms_radius: int = 4, keypoint_threshold: float = 0.005, max_keypoints: int = 1024,
               remove_borders: int = 4) -> Dict[str, List[torch.Tensor]]:
    """The reference's ``SuperPoint.forward`` (estimate_pose/superpoint.py:145-202) on the device.

    ``gray`` is an (H, W) or (n, H, W) float tensor in [0, 1] on a ROCm device, H and W multiples of 8.  Returns the reference's keys as
    lists with one entry per image: ``keypoints`` [N, 2] (x, y) float32, ``scores`` [N], ``descriptors`` [N, 256] — channel-last, where
    the reference holds [256, N].  Order: row-major when at most ``max_keypoints`` (1..4096) survive, else descending score with equal
    scores in row-major order.  The one host synchronisation is the read of the keypoint counts.

    Raises ValueError for CPU tensors (there is no CPU fallback) and for everything the library refuses, the reference's
    ``max_keypoints = -1`` among it."""
    if not torch.is_tensor(gray):
        raise ValueError("superpoint: gray must be a tensor")
    if gray.device.type != "cuda":
        raise ValueError(f"superpoint: needs the image on a ROCm device (got {gray.device}); there is no CPU fallback")
    if gray.dim() not in (2, 3):
        raise ValueError(f"superpoint: need an (H, W) or (n, H, W) grey image, got {tuple(gray.shape)}")
    if not isinstance(weights, MatcherWeights):
        raise ValueError("superpoint: weights must come from load_matcher_weights")
    x = gray.to(torch.float32).contiguous()
    n, H, W = x.shape if x.dim() == 3 else (1, *x.shape)
    lib, dev = _lib.api(), x.device
    with torch.cuda.device(dev):
        packed = weights.packed(dev)
        sizes = [_lib.user_call(_sized, fn, n, H, W) for fn in (lib.car_superpoint_workspace_bytes, lib.car_superpoint_nms_workspace_bytes,
                                                               lib.car_superpoint_select_workspace_bytes)]
        if not 1 <= max_keypoints <= MAX_KEYPOINTS:                     # before anything is allocated by it
            raise ValueError(f"superpoint: max_keypoints = {max_keypoints}, need 1..{MAX_KEYPOINTS} (the reference's -1, \"all\", is not served)")
        work = torch.empty(max(sizes), dtype=torch.uint8, device=dev)
        scores = torch.empty(n, H, W, dtype=torch.float32, device=dev)
        kept = torch.empty_like(scores)
        desc = torch.empty(n, H // 8, W // 8, 256, dtype=torch.float32, device=dev)
        kpts = torch.empty(n, max_keypoints, 2, dtype=torch.float32, device=dev)
        kscores = torch.empty(n, max_keypoints, dtype=torch.float32, device=dev)
        count = torch.empty(n, dtype=torch.int32, device=dev)
        st = _lib.stream()
        _lib.user_call(lib.car_superpoint_dense, x.data_ptr(), n, H, W, packed.data_ptr(), scores.data_ptr(), desc.data_ptr(), work.data_ptr(), sizes[0], st)
        _lib.user_call(lib.car_superpoint_nms, scores.data_ptr(), n, H, W, nms_radius, kept.data_ptr(), work.data_ptr(), sizes[1], st)
        _lib.user_call(lib.car_superpoint_select, kept.data_ptr(), n, H, W, keypoint_threshold, remove_borders, max_keypoints, kpts.data_ptr(),
                       kscores.data_ptr(), count.data_ptr(), work.data_ptr(), sizes[2], st)
        counts = count.cpu().tolist()                                   # the one host synchronisation
        out = {"keypoints": [], "scores": [], "descriptors": []}
        for i, N in enumerate(counts):
            k = kpts[i, :N].contiguous()
            d = torch.empty(N, 256, dtype=torch.float32, device=dev)
            if N:
                _lib.user_call(lib.car_superpoint_sample, k.data_ptr(), N, desc[i].data_ptr(), H // 8, W // 8, d.data_ptr(), st)
            out["keypoints"].append(k)
            out["scores"].append(kscores[i, :N].contiguous())
            out["descriptors"].append(d)
    return out


def _sized(fn, *args) -> int:
    """A size entry's value; 0 (a refused shape) raises the library's message as the argument error it is."""
    size = fn(*args)
    if size == 0:
        raise _lib.CarError(_lib.CAR_E_ARG, fn.__name__)
    return size


def superglue(kpts0, scores0, desc0, kpts1, scores1, desc1, image_shape, weights: MatcherWeights, sinkhorn_iterations: int = 20,
              match_threshold: float = 0.2) -> Dict[str, torch.Tensor]:
    """The reference's ``SuperGlue.forward`` (estimate_pose/superglue.py:230-285) on one pair, on the device.

    ``kpts`` [N, 2] (x, y), ``scores`` [N], ``desc`` [N, 256] per image as ``superpoint`` returns them, at most 1024 keypoints each;
    ``image_shape`` = (H, W) of both images, or ((H0, W0), (H1, W1)).  Returns ``matches0`` [N0], ``matches1`` [N1] (int32, -1 = no
    match), ``matching_scores0``, ``matching_scores1``.  An empty set on either side gives all -1 and zeros without a launch.  Nothing
    waits for the launches."""
    ts = (kpts0, scores0, desc0, kpts1, scores1, desc1)
    if not all(torch.is_tensor(t) for t in ts):
        raise ValueError("superglue: keypoints, scores and descriptors must be tensors")
    dev = kpts0.device
    if dev.type != "cuda" or any(t.device != dev for t in ts):
        raise ValueError(f"superglue: needs all six tensors on one ROCm device (got {[str(t.device) for t in ts]}); there is no CPU fallback")
    if not isinstance(weights, MatcherWeights):
        raise ValueError("superglue: weights must come from load_matcher_weights")
    N0, N1 = len(kpts0), len(kpts1)
    for k, s, d, N in ((kpts0, scores0, desc0, N0), (kpts1, scores1, desc1, N1)):
        if tuple(k.shape) != (N, 2) or tuple(s.shape) != (N,) or tuple(d.shape) != (N, 256):
            raise ValueError(f"superglue: need keypoints [N, 2], scores [N] and descriptors [N, 256], got {tuple(k.shape)}, {tuple(s.shape)}, {tuple(d.shape)}")
    if max(N0, N1) > MAX_GLUE_KEYPOINTS:
        raise ValueError(f"superglue: {N0} and {N1} keypoints, at most {MAX_GLUE_KEYPOINTS} per image are served")
    shapes = tuple(image_shape)
    (H0, W0), (H1, W1) = (shapes, shapes) if isinstance(shapes[0], int) else shapes
    with torch.cuda.device(dev):
        m0 = torch.full((N0,), -1, dtype=torch.int32, device=dev)
        m1 = torch.full((N1,), -1, dtype=torch.int32, device=dev)
        s0 = torch.zeros(N0, dtype=torch.float32, device=dev)
        s1 = torch.zeros(N1, dtype=torch.float32, device=dev)
        out = {"matches0": m0, "matches1": m1, "matching_scores0": s0, "matching_scores1": s1}
        if N0 == 0 or N1 == 0:
            weights.packed_glue(dev)                                   # still refuses weights without a SuperGlue part
            return out
        lib, packed, layers = _lib.api(), weights.packed_glue(dev), len(weights.gnn_layers)
        cross = (ctypes.c_int * layers)(*[int(n == "cross") for n in weights.gnn_layers])
        a = [t.to(torch.float32).contiguous() for t in ts]
        sizes = [_lib.user_call(_sized, fn, N0, N1) for fn in (lib.car_superglue_workspace_bytes, lib.car_superglue_transport_workspace_bytes,
                                                              lib.car_superglue_matches_workspace_bytes)]
        work = torch.empty(max(sizes), dtype=torch.uint8, device=dev)
        mdesc = torch.empty(N0 + N1, 256, dtype=torch.float32, device=dev)
        Z = torch.empty(N0 + 1, N1 + 1, dtype=torch.float32, device=dev)
        st = _lib.stream()
        _lib.user_call(lib.car_superglue_descriptors, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), N0, H0, W0, a[3].data_ptr(), a[4].data_ptr(),
                       a[5].data_ptr(), N1, H1, W1, packed.data_ptr(), layers, cross, mdesc.data_ptr(), work.data_ptr(), sizes[0], st)
        _lib.user_call(lib.car_superglue_transport, mdesc.data_ptr(), N0, mdesc[N0:].data_ptr(), N1, weights.bin_score, sinkhorn_iterations, Z.data_ptr(),
                       work.data_ptr(), sizes[1], st)
        _lib.user_call(lib.car_superglue_matches, Z.data_ptr(), N0, N1, match_threshold, m0.data_ptr(), m1.data_ptr(), s0.data_ptr(), s1.data_ptr(),
                       work.data_ptr(), sizes[2], st)
    return out


def match_pair(gray0: torch.Tensor, gray1: torch.Tensor, weights: MatcherWeights, nms_radius: int = 4, keypoint_threshold: float = 0.005,
               max_keypoints: int = 1024, remove_borders: int = 4, sinkhorn_iterations: int = 20, match_threshold: float = 0.2) -> Dict[str, torch.Tensor]:
    """The reference's ``Matching.forward`` (estimate_pose/glue_match.py:56-84) on two (H, W) grey images in [0, 1] on a ROCm device,
    with the configuration of dataset/load_video_superglue.py:421-432 as the defaults.  Returns the reference's keys for the one pair,
    without its batch dimension: ``keypoints0/1`` [N, 2], ``scores0/1`` [N], ``descriptors0/1`` [N, 256] (channel-last), ``matches0/1``,
    ``matching_scores0/1``.  The one host synchronisation is the read of the keypoint counts."""
    if not (torch.is_tensor(gray0) and torch.is_tensor(gray1)) or gray0.dim() != 2 or gray1.dim() != 2:
        raise ValueError("match_pair: need two (H, W) grey images")
    if gray0.device != gray1.device:
        raise ValueError(f"match_pair: needs both images on one ROCm device (got {gray0.device} and {gray1.device}); there is no CPU fallback")
    if max_keypoints > MAX_GLUE_KEYPOINTS:
        raise ValueError(f"match_pair: max_keypoints = {max_keypoints}, SuperGlue serves at most {MAX_GLUE_KEYPOINTS} keypoints per image")
    args = (weights, nms_radius, keypoint_threshold, max_keypoints, remove_borders)
    if gray0.shape == gray1.shape:
        sp = superpoint(torch.stack([gray0, gray1]), *args)
    else:
        a, b = superpoint(gray0, *args), superpoint(gray1, *args)
        sp = {k: a[k] + b[k] for k in a}
    out = {f"{k}{i}": sp[k][i] for k in ("keypoints", "scores", "descriptors") for i in (0, 1)}
    out.update(superglue(out["keypoints0"], out["scores0"], out["descriptors0"], out["keypoints1"], out["scores1"], out["descriptors1"],
                         (tuple(gray0.shape), tuple(gray1.shape)), weights, sinkhorn_iterations, match_threshold))
    return out
