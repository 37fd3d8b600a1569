"""Training summaries and the validation render (reference summaries.py:15-141, training.py:95-117, 146-231), built on the device.

The reference pulls ``pixel_val`` and the depth to the host, paints the epipolar panel in a Python loop over scenes x views x samples,
and evaluates the attention entropy as a chain of full-size elementwise kernels at every training step.  Here the entropy is one small
reduction whose result stays on the device (``car_attention_entropy``), and the five image panels are built where the frames already
are (``car_colormap``, ``car_epipolar_overlay``, ``car_image_grid``; csrc/car_summary.hip).  There is no CPU fallback:
every function below raises ValueError for tensors that are not on a ROCm device.

``img_summaries`` / ``epi_summary`` keep the reference's signatures, tags and call order, so any object with ``add_scalar(tag, value,
step)`` and ``add_image(tag, chw_image, step)`` serves as the writer — a TensorBoard ``SummaryWriter`` included (untested here: the
package is not installed where this is developed).  ``SummaryLog`` is the built-in writer: scalars as JSON lines, images as PNG files.

``car_image_grid`` restates ``torchvision.utils.make_grid(normalize=True)`` from its documented behaviour; it is pinned to that
restatement (tests/summary_restatement.py), not to the package, which is not installed here either."""
from __future__ import annotations

import ctypes
import json
import os
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib, harness

Tensor = torch.Tensor

PROBE_RAY = 2065                                   # summaries.py:96: the ray whose samples the epipolar panel shows
DEPTH_SCALE = 10.0                                 # summaries.py:36


def _on_device(what: str, *tensors: Tensor) -> torch.device:
    dev = tensors[0].device if torch.is_tensor(tensors[0]) else None
    for t in tensors:
        if not torch.is_tensor(t) or t.device.type != "cuda" or t.device != dev:
            raise ValueError(f"{what}: needs its tensors on one ROCm device; there is no CPU fallback")
    return dev


def _f32(t: Tensor) -> Tensor:
    return t.detach().to(torch.float32).contiguous()


# ---- the four kernels -----------------------------------------------------------------------------------------------------------------
def attention_entropy_sum(at_wt: Tensor, nan_rows_zero: bool) -> Tuple[Tensor, int]:
    """``(sum over the rows of -sum_j w_j log(w_j + 1e-5), rows)`` of ``at_wt`` (..., S): the sum a 0-d float64 device tensor.  A caller
    that renders in chunks adds the sums and divides once (``render_full``)."""
    dev = _on_device("attention_entropy", at_wt)
    w = _f32(at_wt)
    S = w.shape[-1]
    rows = w.numel() // max(S, 1)
    lib = _lib.api()
    with torch.cuda.device(dev):
        n = lib.car_attention_entropy_scratch_doubles(rows, S)
        out = torch.empty((), dtype=torch.float64, device=dev)
        scratch = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
        _lib.user_call(lib.car_attention_entropy, w.data_ptr(), rows, S, int(bool(nan_rows_zero)), out.data_ptr(), scratch.data_ptr(), n, _lib.stream())
    return out, rows


def attention_entropy(at_wt: Tensor, nan_rows_zero: bool = True) -> Tensor:
    """Mean attention entropy of ``at_wt`` (..., S), 1 <= S <= 768, as a 0-d float64 device tensor; nothing waits for the launches.
    ``nan_rows_zero=True`` is the training loop's form (training.py:112-114: a NaN row counts as 0), ``False`` the summary's
    (summaries.py:25-26: a NaN propagates)."""
    total, rows = attention_entropy_sum(at_wt, nan_rows_zero)
    return total / rows


_jet_tables = {}


def _jet_on(dev: torch.device) -> Tensor:
    """The default table on ``dev``, uploaded once: an upload from pageable host memory makes torch wait for the stream, and img_summaries
    promises that nothing of it waits for the device."""
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _jet_tables:
        _jet_tables[key] = _f32(harness.jet_lut()).to(dev)
    return _jet_tables[key]


def colormap(x: Tensor, scale: float = DEPTH_SCALE, lut: Optional[Tensor] = None) -> Tensor:
    """``x`` (N, H, W) -> (N, H, W, 3): matplotlib's colour-map call on ``x / scale`` with the 256-entry table ``lut`` (default: jet)."""
    dev = _on_device("colormap", x)
    if x.dim() != 3:
        raise ValueError(f"colormap: need an (N, H, W) map, got {tuple(x.shape)}")
    v = _f32(x)
    table = _jet_on(dev) if lut is None else _f32(lut).to(dev)
    if tuple(table.shape) != (256, 3):
        raise ValueError(f"colormap: the table must be (256, 3), got {tuple(table.shape)}")
    N, H, W = v.shape
    with torch.cuda.device(dev):
        out = torch.empty(N, H, W, 3, dtype=torch.float32, device=dev)
        _lib.user_call(_lib.api().car_colormap, v.data_ptr(), N, H, W, ctypes.c_float(scale), table.data_ptr(), out.data_ptr(), _lib.stream())
    return out


def epipolar_overlay(trgt: Tensor, ctxt: Tensor, pixel_val: Tensor, at_wt_max: Tensor, uv: Tensor, n_view: int,
                     probe: int = PROBE_RAY) -> Tensor:
    """The epipolar panel (summaries.py:72-136): ``trgt`` (B, H, W, 3), ``ctxt`` (B * n_view, H, W, 3) scene-major, ``pixel_val``
    (B * n_view, R, S, 2), ``at_wt_max`` (B * n_view, R[, 1]) integer, ``uv`` (B, [1,] R, 2); only ray ``probe`` is read.  Returns
    (B + B * n_view, H, W, 3): the targets with the probe pixel marked -1, then the context tiles view-major with the ray's samples
    painted 0 and its arg-max sample -1."""
    dev = _on_device("epipolar_overlay", trgt, ctxt, pixel_val, at_wt_max, uv)
    if trgt.dim() != 4 or trgt.shape[-1] != 3 or ctxt.dim() != 4 or ctxt.shape[1:] != trgt.shape[1:] or ctxt.shape[0] != trgt.shape[0] * n_view:
        raise ValueError(f"epipolar_overlay: need (B, H, W, 3) targets and (B * {n_view}, H, W, 3) context tiles, got {tuple(trgt.shape)} "
                         f"and {tuple(ctxt.shape)}")
    B, H, W, _ = trgt.shape
    if pixel_val.dim() != 4 or pixel_val.shape[0] != B * n_view or pixel_val.shape[-1] != 2:
        raise ValueError(f"epipolar_overlay: pixel_val must be ({B * n_view}, R, S, 2), got {tuple(pixel_val.shape)}")
    rays, S = pixel_val.shape[1:3]
    if at_wt_max.numel() != B * n_view * rays or uv.numel() != B * rays * 2:
        raise ValueError(f"epipolar_overlay: at_wt_max {tuple(at_wt_max.shape)} and uv {tuple(uv.shape)} do not hold {rays} rays per row")
    t, c, pv, u = _f32(trgt), _f32(ctxt), _f32(pixel_val), _f32(uv)
    best = at_wt_max.detach().to(torch.int64).contiguous()
    with torch.cuda.device(dev):
        panel = torch.empty(B * (1 + n_view), H, W, 3, dtype=torch.float32, device=dev)
        _lib.user_call(_lib.api().car_epipolar_overlay, t.data_ptr(), c.data_ptr(), pv.data_ptr(), best.data_ptr(), u.data_ptr(), B, n_view, H, W,
                       rays, int(probe), S, panel.data_ptr(), _lib.stream())
    return panel


def grid_shape(N: int, H: int, W: int) -> Tuple[int, int]:
    """(Hg, Wg) of ``image_grid``'s result: make_grid's nrow = 8, padding = 2; one image comes back unpadded."""
    if N == 1:
        return H, W
    xm = min(8, N)
    return (H + 2) * -(-N // xm) + 2, (W + 2) * xm + 2


def image_grid(x: Tensor, scale_each: bool = False, clamp: Optional[Tuple[float, float]] = None) -> Tensor:
    """``torchvision.utils.make_grid(x, normalize=True, scale_each=scale_each)`` of channel-last images ``x`` (N, H, W, 3), optionally
    clamped first: the planar (3, Hg, Wg) grid in [0, 1] (``grid_shape``), padding 0."""
    dev = _on_device("image_grid", x)
    if x.dim() != 4 or x.shape[-1] != 3:
        raise ValueError(f"image_grid: need (N, H, W, 3) images, got {tuple(x.shape)}")
    v = _f32(x)
    N, H, W, _ = v.shape
    lo, hi = clamp if clamp is not None else (0.0, 0.0)
    lib = _lib.api()
    with torch.cuda.device(dev):
        n = lib.car_image_grid_scratch_floats(N, H, W)
        Hg, Wg = grid_shape(max(N, 1), H, W)
        out = torch.empty(3, Hg, Wg, dtype=torch.float32, device=dev)
        scratch = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
        _lib.user_call(lib.car_image_grid, v.data_ptr(), N, H, W, int(bool(scale_each)), int(clamp is not None), ctypes.c_float(lo), ctypes.c_float(hi),
                       out.data_ptr(), scratch.data_ptr(), n, _lib.stream())
    return out


# ---- the reference's summary functions ------------------------------------------------------------------------------------------------
def _channel_last(tiles: Tensor) -> Tensor:
    """The reference hands NCHW tiles to epi_summary; the kernels take channel-last ones.  Both are accepted."""
    if tiles.dim() == 4 and tiles.shape[-1] != 3 and tiles.shape[1] == 3:
        return tiles.permute(0, 2, 3, 1)
    return tiles


def img_summaries(model, model_input, ground_truth, loss_summaries, model_output, writer, iter, prefix="", img_shape=(98, 144), n_view=1):
    """summaries.py:15-68 with its tags in its order: ``ent``, ``predictions``, ``depth_images``, ``context_images``, ``query_images``,
    ``epipolar_line``, ``out_min``, ``out_max``, ``trgt_min``, ``trgt_max`` (its two prints are dropped).  Images are (3, Hg, Wg) device
    tensors in [0, 1], scalars 0-d device tensors: nothing here waits for the device.  ``model_output`` is a forward's dict or
    ``render_full``'s."""
    Hi, Wi = img_shape
    rgb = model_output["rgb"]
    predictions = rgb.reshape(-1, Hi, Wi, 3)                           # flatten_first_two of (b, 1, H, W, 3)
    if "at_wt" in model_output:
        writer.add_scalar(prefix + "ent", attention_entropy(model_output["at_wt"], nan_rows_zero=False), iter)
    elif "ent_sum" in model_output:                                  # render_full: the chunks' sums, divided once
        writer.add_scalar(prefix + "ent", model_output["ent_sum"] / model_output["ent_rows"], iter)
    writer.add_image(prefix + "predictions", image_grid(predictions, scale_each=False, clamp=(-1.0, 1.0)), iter)

    depth = model_output["depth_ray"].reshape(-1, Hi, Wi)
    writer.add_image(prefix + "depth_images", image_grid(colormap(depth, DEPTH_SCALE), scale_each=True), iter)

    context_images = torch.flatten(model_input["context"]["rgb"], 0, 1)
    writer.add_image(prefix + "context_images", image_grid(context_images, scale_each=False), iter)

    query_images = model_input["query"]["rgb"].reshape(-1, Hi, Wi, 3)
    writer.add_image(prefix + "query_images", image_grid(query_images, scale_each=False), iter)

    epi_summary(model_output, query_images, context_images, writer, iter, prefix=prefix, n_view=n_view)

    clamped = predictions.clamp(-1, 1)
    writer.add_scalar(prefix + "out_min", clamped.min(), iter)
    writer.add_scalar(prefix + "out_max", clamped.max(), iter)
    writer.add_scalar(prefix + "trgt_min", query_images.min(), iter)
    writer.add_scalar(prefix + "trgt_max", query_images.max(), iter)


def epi_summary(model_output, trgt_imgs_tile, ctxt_imgs_tile, writer, iter, prefix="", n_view=1):
    """summaries.py:72-141: the ``epipolar_line`` panel.  The tiles are channel-last (N, H, W, 3) — the reference's NCHW tiles are accepted
    too — and are not modified.  The probe ray is ``model_output['probe']`` when the dict names one (``render_full`` keeps only that
    ray's ``pixel_val`` / ``at_wt_max`` rows), the reference's fixed ray 2065 otherwise; a frame with fewer rays is refused."""
    trgt, ctxt = _channel_last(trgt_imgs_tile), _channel_last(ctxt_imgs_tile)
    pixel_val, at_wt_max, uv = model_output["pixel_val"], model_output["at_wt_max"], model_output["uv"]
    probe = int(model_output.get("probe", PROBE_RAY))
    B = trgt.shape[0]
    uv = uv.reshape(B, -1, 2)
    if probe >= uv.shape[1]:
        raise ValueError(f"epi_summary: probe ray {probe} of a frame with {uv.shape[1]} rays")
    if pixel_val.shape[1] == 1 and uv.shape[1] != 1:                 # the probe's rows only: index them by 0, and take the probe's uv
        uv, probe = uv[:, probe:probe + 1], 0
    panel = epipolar_overlay(trgt, ctxt, pixel_val.to(trgt.device), at_wt_max, uv, n_view, probe)
    writer.add_image(prefix + "epipolar_line", image_grid(panel, scale_each=False), iter)


# ---- the chunked validation render ----------------------------------------------------------------------------------------------------
@torch.no_grad()
def render_full(model, model_input, z, chunk_rays: int = harness.CHUNK_RAYS, probe: int = PROBE_RAY, nan_rows_zero: bool = False) -> Dict[str, Tensor]:
    """The reference's chunked validation render (training.py:157-196) for batches too large for one call: ``chunk_rays`` rays of every
    scene per call (the engine itself groups the scenes of a call when memory is short).  Returns ``rgb`` (b, 1, R, 3), ``depth_ray``
    (b, R, 1), ``valid_mask`` (b, R, 1), ``uv``, the running entropy sum ``ent_sum`` (0-d float64 on the device) with its row count
    ``ent_rows``, and of ``pixel_val`` / ``at_wt_max`` only ray ``probe``'s rows, (b * n_view, 1, S, 2) and (b * n_view, 1, 1), with
    ``probe`` itself.  The full-size ``pixel_val`` and ``at_wt`` of a chunk are dropped as soon as its entropy and probe rows are taken,
    never concatenated.  Rays are independent in the forward, so ``rgb`` and ``depth_ray`` carry the same bits as one call's."""
    uv_full = model_input["query"]["uv"]
    R = uv_full.shape[2]
    if not 0 <= probe < R:
        raise ValueError(f"render_full: probe ray {probe} of a frame with {R} rays")
    if chunk_rays < 1:
        raise ValueError("render_full: chunk_rays must be at least 1")
    keep = ("rgb", "depth_ray", "valid_mask")
    tiles = {k: [] for k in keep}
    probe_pv = probe_best = ent_sum = None
    ent_rows = 0
    query = {k: v for k, v in model_input["query"].items() if k != "rgb"}      # the forward never reads the target colours
    for c0 in range(0, R, chunk_rays):
        c1 = min(R, c0 + chunk_rays)
        out = model({"context": model_input["context"], "query": dict(query, uv=uv_full[:, :, c0:c1])}, z=z, val=True)
        for k in keep:
            tiles[k].append(out[k])
        total, rows = attention_entropy_sum(out["at_wt"], nan_rows_zero)
        ent_sum = total if ent_sum is None else ent_sum + total
        ent_rows += rows
        if c0 <= probe < c1:
            probe_pv = out["pixel_val"][:, probe - c0:probe - c0 + 1].clone()
            probe_best = out["at_wt_max"][:, probe - c0:probe - c0 + 1].clone()
        del out
    res = {k: torch.cat(tiles[k], dim=-2) for k in keep}
    res.update(uv=uv_full, ent_sum=ent_sum, ent_rows=ent_rows, pixel_val=probe_pv, at_wt_max=probe_best, probe=probe)
    return res


# ---- the built-in writer --------------------------------------------------------------------------------------------------------------
class SummaryLog:
    """The writer the training script uses (TensorBoard is optional and not assumed): ``add_scalar`` keeps its value as it comes — a
    device tensor stays un-synced — until ``flush()`` turns all pending values into ``{"tag", "step", "value"}`` lines appended to
    ``<dir>/scalars.jsonl`` with one download; ``add_image`` writes a (3, H, W) image in [0, 1] to ``<dir>/images/<tag>/<step:06d>.png``
    (harness.write_png)."""

    def __init__(self, dir: str):
        self.dir = dir
        os.makedirs(dir, exist_ok=True)
        self._pending: List[tuple] = []

    def add_scalar(self, tag: str, value, step: int) -> None:
        self._pending.append((tag, int(step), value.detach() if torch.is_tensor(value) else value))

    def image_path(self, tag: str, step: int) -> str:
        return os.path.join(self.dir, "images", tag, f"{int(step):06d}.png")

    def add_image(self, tag: str, img, step: int) -> None:
        img = torch.as_tensor(img)
        if img.dim() != 3 or img.shape[0] != 3:
            raise ValueError(f"SummaryLog.add_image: need a (3, H, W) image, got {tuple(img.shape)}")
        path = self.image_path(tag, step)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        harness.write_png(path, torch.nan_to_num(img.detach().float().permute(1, 2, 0)) * 2 - 1)      # write_png maps [-1, 1] to 0..255

    def flush(self) -> None:
        if not self._pending:
            return
        pending, self._pending = self._pending, []
        on_device = [v for _, _, v in pending if torch.is_tensor(v) and v.device.type != "cpu"]
        values = iter(torch.stack([v.reshape(()).double() for v in on_device]).cpu().tolist()) if on_device else iter(())   # the one sync
        with open(os.path.join(self.dir, "scalars.jsonl"), "a") as fh:
            for tag, step, v in pending:
                if torch.is_tensor(v):
                    v = next(values) if v.device.type != "cpu" else float(v)
                fh.write(json.dumps({"tag": tag, "step": step, "value": float(v)}) + "\n")

    def close(self) -> None:
        self.flush()
