"""The one-call route of the render forward (the reference's default configuration): ``car_render_forward`` per batch of rays.  This
module only sizes the calls: rays (and, if need be, scenes) are chunked so that the per-call workspace fits the free device memory (rays
and scenes are independent, so this changes nothing) — integer arithmetic (``scenes_per_lattice``, ``call_size``, ``call_ranges``) kept
apart from ``render``'s allocations, memory queries and calls.
"""
from __future__ import annotations

import ctypes
from typing import Callable, Dict, Iterator, List, Tuple

import torch

from . import _lib
from .engine import _ptr, _stream

Tensor = torch.Tensor


def scenes_per_lattice(b: int, pair_bytes: Callable[[int], int], usable: int) -> int:
    """Scenes per lattice buffer: all ``b`` of them unless ``pair_bytes(b)`` would leave less than half of the ``usable`` bytes for the
    workspace; then halved until a buffer fits that half (or holds one scene)."""
    pg = b
    while pg > 1 and pair_bytes(pg) > usable // 2:
        pg = (pg + 1) // 2
    return pg


def call_size(scenes: int, gs_cap: int, R: int, ws_bytes: Callable[[int, int], int], budget: int) -> Tuple[int, int]:
    """(scenes per call, rays per call) of one lattice group of ``scenes`` scenes x ``R`` rays: at most ``gs_cap`` scenes, halved while
    the workspace ``ws_bytes(scenes, rays)`` of whole scenes exceeds ``budget``; then, if one such call still does not fit, rays in
    whole sample tiles of the fused kernel (24 rays each), sized by the workspace's bytes per ray at 4800 rays."""
    gs = min(gs_cap, scenes)
    while gs > 1 and ws_bytes(gs, R) > budget:
        gs = (gs + 1) // 2
    rc = R
    if ws_bytes(gs, R) > budget:
        per_ray = ws_bytes(gs, 4800) / 4800.0
        rc = int(budget / per_ray) // 48 * 48
        if rc < 48:
            raise RuntimeError(f"forward: {budget / 2**20:.0f} MiB of workspace cannot hold even 48 rays "
                               f"({ws_bytes(gs, 48) / 2**20:.0f} MiB needed): free device memory")
    return gs, rc


def call_ranges(p0: int, p1: int, gs: int, R: int, rc: int) -> Iterator[Tuple[int, int, int, int]]:
    """The (s0, s1, r0, r1) of every call of the lattice group of scenes [p0, p1): ``gs`` scenes x ``rc`` rays each, the last ones ragged."""
    for s0 in range(p0, p1, gs):
        for r0 in range(0, R, rc):
            yield s0, min(p1, s0 + gs), r0, min(R, r0 + rc)


def render(eng, inp, z: List[Tensor], b: int, R: int, debug: bool) -> Dict[str, Tensor]:
    m, lib = eng.m, eng.lib
    V, P = m.n_view, m.npoints
    poses, uv, steps = eng._rays_in(inp, b, R)
    dev = uv.device
    f32 = dict(device=dev, dtype=torch.float32)
    n = b * V
    d_all = eng._dims(b, R, z)
    plan = eng._plan_for(d_all, dev)
    f16 = eng.render_precision == "fp16"
    plan16 = eng._plan16_for(d_all, dev) if f16 else None
    lh, lw, _ = eng._lattice_shape(d_all)
    lattice_scene = V * 2 * lh * lw * 576                                                    # floats per scene

    phases = 1 | 2 | (0 if eng.first_round_parts else 4) | (0 if eng.second_round_merged else 8)

    def ws_bytes(nb, nr):
        return lib.car_workspace_bytes(ctypes.byref(eng._dims(nb, nr, z)))

    def pair_bytes(nb):
        return 4 * lib.car_gmaps_floats(ctypes.byref(eng._dims(nb, R, z)))

    # Scenes per lattice buffer: all of them (2.5 GB per scene at 256 x 256, 5.6 GB at 384 x 384) unless that would leave less than
    # half of the usable device memory for the workspace; then the scenes are rendered in groups, each with its own
    # car_project_maps (re-done on every forward: the one cached buffer holds the last group — a fallback, not a fast path).
    eng._channel_last(z)
    pg = b
    if not eng._pairs.holds([plan, *z], (0, b)):
        # what is live while a group renders: ONE lattice buffer (the previous group's is dropped before the next is allocated, below)
        # and the workspace.  The cached buffer and workspace of an earlier forward count as available because both are released
        # before this forward allocates (a stale workspace sized for another split would otherwise sit beside the new pair)
        eng._pairs.drop()
        if pair_bytes(b) > (eng._free_budget(dev)) // 2:
            eng._work = None                                       # grouped fallback: start from everything this engine can free
        usable = eng._free_budget(dev)
        if eng.max_pair_bytes is not None:
            usable = min(usable, 2 * int(eng.max_pair_bytes))
        pg = scenes_per_lattice(b, pair_bytes, usable)

    # inside a lattice group — scenes per call: any number (the fused kernel addresses the lattice of ONE view and padding mode with
    # 32-bit offsets); max_level_bytes lets tests force smaller calls.  Rays per call: the workspace (~0.44 MB per ray at 64 samples)
    # must fit the free memory.  Rays and scenes are independent, so every split is exact.
    gs_cap = pg if eng.max_level_bytes is None else max(1, min(pg, eng.max_level_bytes // (4 * lattice_scene)))

    out = {"rgb": torch.empty(b, 1, R, 3, **f32), "valid_mask": torch.empty(b, R, 1, **f32), "depth_ray": torch.empty(b, R, 1, **f32),
           "at_wt": torch.empty(n, R, P, **f32), "at_wt_max": torch.empty(n, R, 1, device=dev, dtype=torch.int32),
           "coords": torch.empty(n, R, 9, **f32), "pixel_val": torch.empty(n, R, P, 2, **f32)}
    lead = {"rgb": 1, "valid_mask": 1, "depth_ray": 1, "at_wt": V, "at_wt_max": V, "coords": V, "pixel_val": V}   # rows per scene
    order = ("rgb", "valid_mask", "depth_ray", "at_wt", "at_wt_max", "coords", "pixel_val")
    st = _stream()
    calls = 0
    d_last = None
    eng.last_pair_groups = -(-b // pg)
    pair = work = None
    for p0 in range(0, b, pg):
        p1 = min(b, p0 + pg)
        if pg < b:
            # several lattice groups (memory pressure): the previous group's buffer must be gone before the next one is allocated —
            # _pair_for drops the engine's reference, this drops the loop's — and the workspace is re-sized against what is then free
            pair = work = None
            eng._work = None
        pair, d_pair = eng._pair_for(plan, z, dev, p0, p1, R)
        gmeta_ptr = pair.data_ptr() + 4 * lib.car_gmeta_offset(ctypes.byref(d_pair))
        gs, rc = call_size(p1 - p0, gs_cap, R, ws_bytes, eng._workspace_budget(dev))
        need = ws_bytes(gs, min(rc, R))
        if eng._work is None or eng._work.numel() * 4 < need:
            eng._work = None
            eng._work = torch.empty(need // 4, **f32)
        work = eng._work
        for s0, s1, r0, r1 in call_ranges(p0, p1, gs, R, rc):
            d = eng._dims(s1 - s0, r1 - r0, z)
            whole = (r0 == 0 and r1 == R)
            if whole:
                tgt = {k: out[k][s0 * lead[k]:s1 * lead[k]] for k in order}            # contiguous scene slices: written in place
                uv_c = uv[s0:s1]
            else:
                tgt = {k: torch.empty((s1 - s0) * lead[k], r1 - r0, *out[k].shape[2 if k != "rgb" else 3:],
                                      device=dev, dtype=out[k].dtype) for k in order}
                uv_c = uv[s0:s1, r0:r1].contiguous()
            ci = _lib.CarInputs()
            ci.poses = poses.data_ptr() + 4 * 96 * s0 * V
            ci.uv = uv_c.data_ptr()
            ci.lattice = pair.data_ptr() + 4 * (s0 - p0) * lattice_scene
            ci.gmeta = gmeta_ptr
            ci.steps = steps.data_ptr()
            co = _lib.CarOutputs(*[tgt[k].data_ptr() for k in order])
            if f16:
                lib.car_render_forward_f16(ctypes.byref(d), _ptr(plan), _ptr(plan16), ctypes.byref(ci), ctypes.byref(co), _ptr(work), work.numel() * 4, phases, st)
            else:                                       # phases == 3 is car_render_forward's own call
                lib.car_render_forward_phase(ctypes.byref(d), _ptr(plan), ctypes.byref(ci), ctypes.byref(co), _ptr(work), work.numel() * 4, phases, st)
            if not whole:
                for k in order:
                    dst = out[k][:, 0] if k == "rgb" else out[k]
                    dst[s0 * lead[k]:s1 * lead[k], r0:r1] = tgt[k]
            calls += 1
            d_last = d
    eng.last_calls = calls
    eng.last_precision = "fp16" if f16 else "fp32"
    res = eng._outputs(inp, z, out, debug)
    if debug:
        if calls != 1:
            raise RuntimeError("debug=True needs the forward to fit one car_render_forward call (intermediates live in its workspace)")

        def ws(name, *shape):
            off, cnt = ctypes.c_size_t(), ctypes.c_size_t()
            lib.car_workspace_find(ctypes.byref(d_last), name.encode(), ctypes.byref(off), ctypes.byref(cnt))
            return work[off.value:off.value + cnt.value].view(*shape).clone()
        res["stages"] = {"rays": ws("rays", n, R, 12), "pt": ws("pt", n, R, P, 3), "local_coords": None,
                         "g": ws("g", n, R, P, 16), "interp_val": ws("e", n, R, P, 576),
                         "z1": ws("z1", b, R, 288),
                         "at_wt2": ws("at_wt2", n, R, P) if m.repeat_attention else None, "poses": poses}
    return res
