#!/usr/bin/env python
"""Every size and offset entry of the C ABI over a fixed grid of shapes, as one JSON table.

Per entry the grid holds the smallest accepted shape, one odd shape (non-multiples of every granule: N0 = 3, N1 = 5, S = 33, H = 7
hypotheses, ...), the workload's shape and one refused shape (0 or (size_t)-1 comes back).  The sizes are public: a caller allocates by
them, so a change of a layout must leave every row as it is.  ``tests/golden/workspace_sizes.json`` is this table as the library stood
before the layouts moved onto csrc/car_workspace.h; tests/test_workspace_sizes.py requires the tree's library to reproduce it.

    python tools/dump_workspace_sizes.py [--lib libcar_hip.so] [--out table.json]

The library loads without a device: no entry here touches one.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cross_attention_renderer_amd import _lib  # noqa: E402

# the one-call forward's dims: (b, V, R, P, H, W, ((level_c, level_h = level_w), ...))
DIMS = {
    "smallest": (1, 2, 1, 2, 2, 2, ((560, 1), (12, 1), (4, 1))),
    "odd": (3, 2, 33, 33, 32, 32, ((560, 8), (12, 16), (4, 32))),
    "workload": (1, 2, 8192, 64, 256, 256, ((256, 64), (256, 128), (64, 256))),
    "refused": (1, 3, 8192, 64, 256, 256, ((256, 64), (256, 128), (64, 256))),          # n_view = 3
}
FINDABLE = ("rays", "e", "g", "logit", "logit2", "pt", "at_wt2", "ebar", "z1", "uh", "part", "phi_x", "nope")
DIM_ENTRIES = ("car_plan_bytes", "car_plan_f16_bytes", "car_workspace_bytes", "car_gmaps_floats", "car_gmeta_offset")

# the binned scatter: (level_h, level_w, n_levels, n_maps, pts, n_gathers)
SCATTER = [((1,), (1,), 1, 1, 1, 1), ((5, 4), (3, 4), 2, 2, 7, 2), ((64, 128, 256), (64, 128, 256), 3, 2, 8192 * 64, 2), ((5, 4), (3, 4), 0, 2, 7, 2)]

NEVER_REFUSES = ("car_linear_x3_packed_floats",)                                        # a formula of K and N alone: its fourth row is a degenerate K

IMAGES = [(1, 16, 16), (3, 17, 33), (1, 256, 256), (1, 8, 8)]                           # LPIPS: B, H, W
MAPS = [(1, 1, 1), (3, 5, 7), (2, 256, 256), (0, 1, 1)]                                 # n, H, W of a score map
PAIRS = [(1, 1), (3, 5), (1024, 1024), (0, 5)]                                          # SuperGlue: N0, N1
WIDTHS = [(64, 64), (3, 64), (512, 512), (64, 100)]                                     # a 3 x 3 convolution's K, N
GRID = {
    "car_fused_blob_floats": [()], "car_fused_bias_floats": [()], "car_kq_tail_floats": [()], "car_kq_bias_floats": [()],
    "car_round2_packed_floats": [()], "car_round2_bias_floats": [()], "car_round2q_packed_floats": [()], "car_round2q_bias_floats": [()],
    "car_lpips_packed_floats": [()], "car_lpips_backward_packed_floats": [()], "car_frames_table_ints": [()],
    "car_superpoint_packed_floats": [()],
    "car_linear_packed_floats": [(1, 1), (33, 7), (256, 576), (0, 4)],
    "car_linear_x3_packed_floats": [(32, 4), (36, 33), (768, 3072), (0, 4)],
    "car_chain_packed_floats": [(1, 1), (33, 7), (288, 128), (0, 4)],
    "car_conv3x3_packed_floats": WIDTHS,
    "car_conv3x3_backward_packed_floats": WIDTHS,
    "car_ssim_scratch_doubles": [(1, 11, 11, 1), (3, 13, 17, 3), (1, 256, 256, 3), (1, 10, 10, 3)],
    "car_lpips_workspace_bytes": IMAGES,
    "car_lpips_head_scratch_doubles": IMAGES,
    "car_lpips_train_workspace_bytes": IMAGES,
    "car_lpips_train_layer_offset": [(*s, l) for s in IMAGES for l in range(13)] + [(1, 16, 16, 13), (1, 16, 16, -1)],
    "car_attention_entropy_scratch_doubles": [(1, 1), (33, 33), (8192, 128), (0, 1)],
    "car_image_grid_scratch_floats": [(1, 1, 1), (3, 5, 7), (8, 256, 256), (0, 1, 1)],
    "car_essential_workspace_bytes": [(5, 1), (7, 7), (1024, 2048), (4, 7)],
    "car_superpoint_workspace_bytes": [(1, 8, 8), (3, 24, 40), (2, 256, 256), (1, 12, 8)],
    "car_superpoint_nms_workspace_bytes": MAPS,
    "car_superpoint_select_workspace_bytes": MAPS,
    "car_superglue_packed_floats": [(1,), (3,), (18,), (0,)],
    "car_superglue_workspace_bytes": PAIRS,
    "car_superglue_transport_workspace_bytes": PAIRS,
    "car_superglue_matches_workspace_bytes": PAIRS,
    "car_mha_workspace_bytes": [(1, 1, 1), (3, 33, 5), (2, 257, 12), (1, 0, 1)],
    "car_vit_workspace_bytes": [(1, 1, 64), (3, 33, 192), (2, 257, 768), (1, 33, 65)],
    "car_vit_packed_floats": [(64, 1), (192, 3), (768, 12), (65, 1)],
    "car_vit_packed_offset": [(dim, item) for dim in (64, 192, 768) for item in range(13)] + [(64, 13), (65, 0)],
}


def bind(path: str) -> ctypes.CDLL:
    """A library by its path (the tree's, or another build's) with _lib's prototypes."""
    lib = ctypes.CDLL(path)
    for name, (res, args) in {**_lib.SIGNATURES, **_lib.MATCH_SIGNATURES, **_lib.ENCODER_SIGNATURES}.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def size_entries():
    """Names of all entries that return a size_t, and car_workspace_find, which returns an offset and a count."""
    table = {**_lib.SIGNATURES, **_lib.MATCH_SIGNATURES, **_lib.ENCODER_SIGNATURES}
    return sorted(n for n, (res, _) in table.items() if res is ctypes.c_size_t) + ["car_workspace_find"]


def car_dims(spec) -> "_lib.CarDims":
    d = _lib.CarDims()
    d.b, d.V, d.R, d.P, d.H, d.W, levels = spec
    d.n_levels, d.repeat_attention = len(levels), 1
    for l, (c, h) in enumerate(levels):
        d.level_c[l], d.level_h[l], d.level_w[l] = c, h, h
    return d


def rows(lib: ctypes.CDLL):
    """[{"entry", "args", "value"}, ...] in a fixed order; car_workspace_find's value is [status, offset, count]."""
    out = []
    for name in sorted(GRID):
        for args in GRID[name]:
            out.append({"entry": name, "args": list(args), "value": getattr(lib, name)(*args)})
    for shape, spec in DIMS.items():
        d = car_dims(spec)
        for name in DIM_ENTRIES:
            out.append({"entry": name, "args": [shape], "value": getattr(lib, name)(ctypes.byref(d))})
        for tensor in FINDABLE:
            off, cnt = ctypes.c_size_t(), ctypes.c_size_t()
            code = lib.car_workspace_find(ctypes.byref(d), tensor.encode(), ctypes.byref(off), ctypes.byref(cnt))
            out.append({"entry": "car_workspace_find", "args": [shape, tensor], "value": [code, off.value, cnt.value] if code == 0 else [code, 0, 0]})
    for hs, ws, n_levels, n_maps, pts, n_gathers in SCATTER:
        value = lib.car_scatter_workspace_bytes((ctypes.c_int * len(hs))(*hs), (ctypes.c_int * len(ws))(*ws), n_levels, n_maps, pts, n_gathers)
        out.append({"entry": "car_scatter_workspace_bytes", "args": [list(hs), list(ws), n_levels, n_maps, pts, n_gathers], "value": value})
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", default=_lib.LIB_PATH, help="the library to ask (default: the tree's)")
    ap.add_argument("--out", default=None, help="write the table here instead of to standard output")
    a = ap.parse_args()
    text = "[\n" + ",\n".join(json.dumps(r) for r in rows(bind(a.lib))) + "\n]\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
