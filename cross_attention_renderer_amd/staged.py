"""The stage-by-stage route of the render forward: every configuration the one-call route does not take —
also its A/B partner in the tests — and, with a ``Saved`` record, the training forward (training.render_train).  ``forward`` is the
sequence of the stages below; each holds its inference form beside its training form.
"""
from __future__ import annotations

import collections
import ctypes
import dataclasses
from typing import Dict, List, Optional

import torch

from . import _lib
from .engine import ACCUM, PLACE_OTHER2, PLACE_OWN, PLACE_PLAIN, RELU_IN, RELU_OUT, PackedLinear, _levels, _mode, _ptr, _round_up, _stream

Tensor = torch.Tensor


@dataclasses.dataclass(slots=True)
class Saved:
    """What the training forward keeps for its backward (training._RenderTrain).  S = b V R P samples, bR = b R rays, C the pyramid's
    channels, Ce the width of e, Dl = latent_dim, hid the decoder's width.  A field is None (0) in the modes that do not set it."""
    maps: Optional[List[Tensor]] = None        # the channel-last pyramid, [b V, H_l, W_l, C_l] per level: every mode
    Ce: int = 0                                # width of e: every mode
    ld_phi: int = 0                            # row stride of phi_x: every mode
    ld_rows: int = 0                           # row stride of enc_rows: concat2, concat3, single
    pixel_val: Optional[Tensor] = None         # [b V, R, P, 2] sample positions in the own view: every mode
    enc_rows: Optional[Tensor] = None          # input rows of the first per-sample layer: [S V, ld_rows] (concat2), [S 3, ld_rows] (concat3: the exchange rows), [S, ld_rows] (single)
    h1: Optional[Tensor] = None                # [S V, C] (concat2) / [S 3, C] (concat3): query_encode_latent's activations
    grid_other: Optional[Tensor] = None        # [b, V, R, P, 2] where the other line's points land: concat2
    cross: Optional[list] = None               # [(context c, view o, component k, grid [b, R P, 2])] of every cross-view gather: concat3
    e: Optional[Tensor] = None                 # [S, Ce]: every mode
    g: Optional[Tensor] = None                 # [S, 16] local coordinates: every mode
    k1: Optional[Tensor] = None                # [S, 128] key_map's activations: every mode
    key: Optional[Tensor] = None               # [S, 128]: every mode
    q1: Optional[Tensor] = None                # [S, 128] query_embed's activations: every mode
    q: Optional[Tensor] = None                 # [S, 128]: every mode
    pt: Optional[Tensor] = None                # [b V, R, P, 3] sample points: every mode
    poses: Optional[Tensor] = None             # [b V, 96] pose records: every mode
    at_wt: Optional[Tensor] = None             # [b V, R, P] first round's weights: every mode
    ebar1: Optional[Tensor] = None             # [bR, Ce] first round's average: every mode
    z1: Optional[Tensor] = None                # [bR, Dl]: repeat_attention
    hb: Optional[Tensor] = None                # [bR, 128] encode_latent's output: repeat_attention
    k1r: Optional[Tensor] = None               # [S, 128] second round's hidden layer: repeat_attention
    key2: Optional[Tensor] = None              # [S, 128] second round's keys: repeat_attention
    at_wt2: Optional[Tensor] = None            # [b V, R, P] second round's weights: repeat_attention
    ebar2: Optional[Tensor] = None             # [bR, Ce] second round's average: repeat_attention
    zrep: Optional[Tensor] = None              # [bR, V Dl] the latent, once per view: every mode
    phi_x: Optional[Tensor] = None             # [bR, ld_phi] ray coordinates: every mode
    xas: Optional[List[Tensor]] = None         # [bR, hid] per block: its input state: every mode
    nets: Optional[List[Tensor]] = None        # [bR, hid] per block: its hidden activation: every mode
    dec_out: Optional[Tensor] = None           # [bR, hid] the decoder's final state (phi.lin_out's input): every mode
    valid: Optional[Tensor] = None             # [b, R, 1] valid mask: every mode


# What the stages of one forward share: the engine, the training forward's record (None: inference), the sizes (n = b V maps, S = b V R P
# samples, bR = b R rays, C the pyramid's channels, Ce the width of e), engine._mode, proj (the first point-MLP layer per texel:
# car_gather_encode), kmajor (e component-major [S, 3, C/2]: the inference path of _encode_three_views), the packed layers, the channel-last
# pyramid, the pose records and sample steps (a3), the tensor options and the launch stream.
_Run = collections.namedtuple("_Run", "eng save b V R P n S bR C Ce mode proj kmajor pk maps poses steps f32 st")


def forward(eng, inp, z: List[Tensor], debug: bool = False, save: Optional[Saved] = None) -> Dict[str, Tensor]:
    """The stage-by-stage forward of every configuration the one-call route does not take.

    ``save=None``: inference, with the fused stage kernels the engine's switches select and buffers reused where nothing is kept.
    ``save`` a record: the training forward (training.render_train) — the literal forms (gather -> GEMM, five key / query launches, the
    unfused second round, a copy of the decoder's state per block), every activation its backward reads stored into ``save``."""
    m = eng.m
    keep = save is not None
    dev = inp["query"]["uv"].device
    b, V = inp["context"]["rgb"].shape[:2]
    R = inp["query"]["uv"].shape[2]
    # a3: pose algebra on the host, exactly the reference's torch calls
    poses, uv, steps = eng._rays_in(inp, b, R)
    pk = eng._weights(dev)
    maps = eng._channel_last(z)
    C = sum(t.shape[3] for t in maps)
    mode = _mode(m)
    P = m.npoints
    r = _Run(eng=eng, save=save, b=b, V=V, R=R, P=P, n=b * V, S=b * V * R * P, bR=b * R, C=C, Ce=V * (C // 2) if mode in ("concat2", "concat3") else C,
             mode=mode, proj=mode == "concat2" and eng.project_maps and not keep, kmajor=mode == "concat3" and eng.project_maps and not keep,
             pk=pk, maps=maps, poses=poses, steps=steps, f32=dict(device=dev, dtype=torch.float32), st=_stream())
    rays, coords9, phi_x, ld_phi, pixel_val, pt, g, grid_in, pt_in, x1, ld1 = _rays_and_samples(r, uv)
    if mode == "concat2":
        e = _e_concat2(r, pixel_val, grid_in, x1, ld1)
    elif mode == "concat3":
        e = _encode_three_views(r, pixel_val, x1, pt_in)
    elif mode == "single":
        e = _e_single(r, pixel_val, x1, ld1)
    else:
        e = _e_plain(r, pixel_val)
    x1 = None
    q, key, logit1 = _keys_and_queries(r, e, g)
    at_wt, at_wt2, depth, amax, zrep = _attention_rounds(r, e, g, q, key, logit1, pt)
    rgb, valid = _decode(r, phi_x, ld_phi, zrep, rays)
    if keep:
        save.maps, save.Ce, save.ld_phi, save.pixel_val, save.e, save.g, save.pt, save.poses = maps, r.Ce, ld_phi, pixel_val, e, g, pt, poses
    out = eng._outputs(inp, z, dict(rgb=rgb, valid_mask=valid, depth_ray=depth, at_wt=at_wt, at_wt_max=amax, coords=coords9,
                                    pixel_val=pixel_val), debug)
    if debug:
        n, S, Ce, Dl = r.n, r.S, r.Ce, m.latent_dim
        out["stages"] = {"rays": rays, "pt": pt.view(n, R, P, 3),
                         "local_coords": g.view(n, R, P, 16),
                         # the reference's channel order e[s, 3 ch + k] (models.py:446) when e was kept component-major
                         "interp_val": (e.view(S, 3, Ce // 3).permute(0, 2, 1).reshape(n, R, P, Ce) if r.kmajor else e.view(n, R, P, Ce)),
                         "z_final": zrep[:, :Dl].reshape(b, R, Dl), "at_wt2": at_wt2, "poses": poses}
    return out


def _rays_and_samples(r: _Run, uv: Tensor):
    """a4-a6: rays (constant with respect to every parameter, like the rest of the geometry);  a6, a8, a9, a13: samples.  Beside the
    geometry: grid_in (concat2), pt_in (concat3) and the input rows x1 [.., ld1] of the first per-sample layer with their point channels
    filled in (None, 0: no_latent_concat)."""
    m, lib, mode = r.eng.m, r.eng.lib, r.mode
    b, n, R, P, V, S, C = r.b, r.n, r.R, r.P, r.V, r.S, r.C
    rays = torch.empty(n, R, 12, **r.f32)
    coords9 = torch.empty(n, R, 9, **r.f32)
    ld_phi = _round_up(9 * V, 4)
    phi_x = torch.zeros(r.bR, ld_phi, **r.f32)
    lib.car_ray_setup(_ptr(r.poses), _ptr(uv), b, V, R, m.H, m.W, P, int(m.no_sample), _ptr(r.steps), _ptr(rays), _ptr(coords9), _ptr(phi_x), ld_phi, r.st)
    pixel_val = torch.empty(n, R, P, 2, **r.f32)
    pt = torch.empty(n, R, P, 3, **r.f32)
    g = torch.empty(S, 16, **r.f32)
    grid_in = torch.empty(n, R, P, V, 2, **r.f32) if mode == "concat2" else None
    pt_in = torch.empty(n, R, P, V, 3, **r.f32) if mode == "concat3" else None
    x1, ld1, col = None, 0, 0
    if r.proj or mode == "concat3":
        ld1 = 4                                   # only the 3 point channels: [S*V, 4]; the three-view route assembles its rows below
        x1 = torch.zeros(S * V, ld1, **r.f32)
    elif mode in ("concat2", "single"):
        col = C                                   # features in [0, C), point channels in [C, C + 3) (two views) or [C, C + 6) (one)
        ld1 = _round_up(C + (3 if mode == "concat2" else 6), 32)
        x1 = torch.empty(S * V, ld1, **r.f32)
        if r.save is not None:
            x1[:, C + (3 if mode == "concat2" else 6):].zero_()     # the row padding: the backward reads whole rows
    lib.car_sample_setup(_ptr(r.poses), _ptr(rays), _ptr(r.steps), b, V, R, P, m.H, m.W, int(m.no_sample),
                         _ptr(pixel_val), _ptr(pt), _ptr(g), _ptr(grid_in), _ptr(x1), ld1, col, _ptr(pt_in), r.st)
    return rays, coords9, phi_x, ld_phi, pixel_val, pt, g, grid_in, pt_in, x1, ld1


# ---------------------------------------------------------------------- a7, a9-a11: per-sample features e, one function per mode
def _e_concat2(r: _Run, pixel_val: Tensor, grid_in: Tensor, x1: Tensor, ld1: int) -> Tensor:
    eng, V, S, C = r.eng, r.V, r.S, r.C
    pts = r.R * r.P
    grid_other = None
    if r.proj:
        gmaps, wpt = eng._projected_maps(r.maps, pixel_val.device)
        h1 = torch.empty(S * V, C, **r.f32)
        eng.gather_encode(gmaps, wpt, pixel_val, grid_in, x1, V, pts, h1, C)
    else:
        eng.gather(r.maps, pixel_val, pts, 0, PLACE_OWN, V, x1, ld1, 0, run=r.P)
        gi = grid_in.view(r.b, V, r.R, r.P, V, 2)
        # pixel_val_stack (models.py:316): map (b, s) is sampled where the *other* line's points land in view s
        grid_other = torch.stack([gi[:, 1, :, :, 0], gi[:, 0, :, :, 1]], dim=1).contiguous()
        eng.gather(r.maps, grid_other, pts, 1, PLACE_OTHER2, V, x1, ld1, 0, run=r.P)
        h1 = torch.empty(S * V, C, **r.f32)
        eng.linear(x1, ld1, r.pk["query_encode_latent"], h1, C, S * V, RELU_OUT)
    e = torch.empty(S, r.Ce, **r.f32)
    eng.linear(h1, C, r.pk["query_encode_latent_2"], e, C // 2, S * V)
    if r.save is not None:
        r.save.enc_rows, r.save.ld_rows, r.save.h1, r.save.grid_other = x1, ld1, h1, grid_other
    return e


def _e_single(r: _Run, pixel_val: Tensor, x1: Tensor, ld1: int) -> Tensor:
    r.eng.gather(r.maps, pixel_val, r.R * r.P, 0, PLACE_PLAIN, r.V, x1, ld1, 0, run=r.P)
    e = torch.empty(r.S, r.Ce, **r.f32)
    r.eng.linear(x1, ld1, r.pk["update_val_merge"], e, r.Ce, r.S)
    if r.save is not None:
        r.save.enc_rows, r.save.ld_rows = x1, ld1
    return e


def _e_plain(r: _Run, pixel_val: Tensor) -> Tensor:
    e = torch.empty(r.S, r.Ce, **r.f32)                            # no_latent_concat: the gathered features are e
    r.eng.gather(r.maps, pixel_val, r.R * r.P, 0, PLACE_PLAIN, r.V, e, r.Ce, 0, run=r.P)
    return e


def _exchange_lattice(eng, gmaps, ptrs, hs, ws, n_maps, C, dev):
    """The projected levels of the three-view exchange summed on their common lattice (car_merge_lattice), cached on those levels;
    None when the levels have no common lattice, the channel count is not the lattice kernels' 576, or it would not fit."""
    if C != 576:
        return None

    def build():
        L = len(gmaps)
        lh, lw, lpad = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        # the shape query on the raw handle: a refusal (no common lattice) is an answer here, not an error
        if _lib.load().car_merge_lattice(ptrs, hs, ws, L, n_maps, None, ctypes.byref(lh), ctypes.byref(lw), ctypes.byref(lpad), _stream()) != 0:
            return None
        floats = n_maps * 2 * lh.value * lw.value * C
        if n_maps * 2 * lh.value * lw.value >= 2 ** 31 - 1 or floats * 4 > eng._free_budget(dev) // 2:
            return None
        lattice = torch.empty(floats, device=dev, dtype=torch.float32)
        gmax = torch.empty(1, device=dev, dtype=torch.float32)     # largest |lattice value|: taken in the merge's own pass
        eng.lib.car_merge_lattice_max(ptrs, hs, ws, L, n_maps, _ptr(lattice), _ptr(gmax), _stream())
        return lattice, lh.value, lw.value, lpad.value, gmax
    return eng._xlat.get(gmaps, (), build)


def _encode_three_views(r: _Run, pixel_val: Tensor, ptenc: Tensor, pt_in: Tensor) -> Tensor:
    """Cross-view exchange for three context views (models.py:345-475), restated literally: for the samples of context c
    the row is the channel-interleaved concatenation of enc(own features, point in frame c) and, for every other view o
    in ascending order, enc(features of view o where context o's points — moved into frame c, projected with view o's
    intrinsics — land in image o, those points in frame c).  All arithmetic is in HIP kernels (gather, projection, the two
    1x1 layers); torch only moves rows into place.  The training forward saves the 579-wide rows, the first layer's activations and
    every cross-view gather's grid (training.render_train)."""
    if r.kmajor:
        return _exchange_projected(r, pixel_val, ptenc, pt_in)
    eng, lib, maps, poses, sv = r.eng, r.eng.lib, r.maps, r.poses, r.save
    b, P, C, H, W = r.b, r.P, r.C, r.eng.m.H, r.eng.m.W
    V, pts = 3, r.R * r.P
    S = b * V * pts
    f32 = r.f32
    ld = _round_up(C + 3, 32)
    rows = torch.empty(S * 3, ld, **f32)
    rv = rows.view(b, V, pts, 3, ld)                    # [scene, context c, point, component k, channel]
    pe = ptenc.view(b, V, pts, V, 4)                    # tanh(nan_to_num(T_s pt)/5): [scene, context, point, frame s]
    pin = pt_in.view(b, V, pts, V, 3)
    tmp = torch.empty(S, C, **f32)
    eng.gather(maps, pixel_val, pts, 0, PLACE_PLAIN, V, tmp, C, 0, run=P)
    rv[:, :, :, 0, :C] = tmp.view(b, V, pts, C)
    per_view = [[t.view(b, V, *t.shape[1:])[:, o].contiguous() for t in maps] for o in range(V)]
    tmp2 = torch.empty(b * pts, C, **f32)
    grid = torch.empty(b, pts, 2, **f32)
    cross = []
    for c in range(V):
        rv[:, c, :, 0, C:C + 3] = pe[:, c, :, c, :3]
        k = 1
        for o in range(V):
            if o == c:
                continue
            q = pin[:, o, :, c, :].contiguous()         # context o's points expressed in frame c
            lib.car_project_points(_ptr(poses), _ptr(q), b, pts, V, o, H, W, _ptr(grid), _stream())
            eng.gather(per_view[o], grid, pts, 1, PLACE_PLAIN, 1, tmp2, C, 0, run=P)
            if sv is not None:
                cross.append((c, o, k, grid.clone()))
            rv[:, c, :, k, :C] = tmp2.view(b, pts, C)
            rv[:, c, :, k, C:C + 3] = pe[:, o, :, c, :3]
            k += 1
    h1 = torch.empty(S * 3, C, **f32)
    eng.linear(rows, ld, r.pk["query_encode_latent"], h1, C, S * 3, RELU_OUT)
    enc = torch.empty(S * 3, C // 2, **f32)
    eng.linear(h1, C, r.pk["query_encode_latent_2"], enc, C // 2, S * 3)
    if sv is not None:
        sv.enc_rows, sv.ld_rows, sv.h1, sv.cross = rows, ld, h1, cross
    # channel index = ch*3 + k (torch.cat on dim 2 then flatten(1, 2), models.py:446)
    return enc.view(S, 3, C // 2).permute(0, 2, 1).contiguous().view(S, 3 * (C // 2))


def _exchange_projected(r: _Run, pixel_val: Tensor, ptenc: Tensor, pt_in: Tensor) -> Tensor:
    """The exchange at inference: the first layer applied per texel (car_project_maps' arithmetic, as on the two-view route): the
    579 -> 576 GEMM over 3 S rows — two thirds of this variant's FLOPs — becomes one gather over the projected pyramid with an explicit
    row list.  Leaves e component-major [S, 3, C/2]: the consumers' weights are permuted (engine._weights)."""
    eng, lib, C = r.eng, r.eng.lib, r.C
    b, V, R, P, pts, n = r.b, 3, r.R, r.P, r.R * r.P, r.b * 3
    S = n * pts
    dev = pixel_val.device
    f32 = r.f32
    gmaps, wpt = eng._projected_maps(r.maps, dev)
    # the row lists (map | padding mode, grid point, point encoding per (sample, component)) in one launch (car_exchange_rows)
    src = torch.empty(b, V, pts, 3, dtype=torch.int32, device=dev)
    rgrid = torch.empty(b, V, pts, 3, 2, **f32)
    rpe = torch.empty(b, V, pts, 3, 4, **f32)
    lib.car_exchange_rows(_ptr(r.poses), _ptr(pixel_val), _ptr(pt_in), _ptr(ptenc), b, V, pts, eng.m.H, eng.m.W, _ptr(src), _ptr(rgrid), _ptr(rpe), _stream())
    ptrs, _, hs, ws, L = _levels(gmaps)
    lat = _exchange_lattice(eng, gmaps, ptrs, hs, ws, n, C, dev)
    layer2 = r.pk["query_encode_latent_2"]
    if lat is not None and eng.fuse_exchange == "rows" and not eng.linear_flags and C == 576:
        # the fused per-sample kernel's source pass over the exchange's rows (car_fused_rows): its gather machinery and W2 in one
        # launch, e written [S, 3, 288]; the lattice's largest magnitude (the first layer's fp16 scale) is taken once per lattice
        lattice, lh, lw, lpad, gmax = lat
        blob, fbias, fwpt = eng._exchange_pack(dev)
        enc = torch.empty(S * 3, C // 2, **f32)
        if eng._ran(lib.car_fused_rows, _ptr(lattice), lh, lw, lpad, _ptr(gmax), _ptr(fwpt), _ptr(blob), _ptr(fbias), _ptr(src), _ptr(rgrid), _ptr(rpe),
                    n, R, P, 3, _ptr(enc), _stream()):
            return enc.view(S, 3 * (C // 2))
        eng.fuse_exchange = True                           # LDS reservation refused: the gather-fed linear kernel, then two launches
    if lat is not None and eng.fuse_exchange and eng.linear_x3 and not eng.linear_flags and layer2.x3 is not None:
        # first AND second exchange layer in one kernel: the lattice rows are gathered 32 channels at a time into the matrix pipe's
        # operands, the 576-wide rows (2.3 KB x 3 S) are never written (csrc/car_linear16.hip, GATHER instance; bit-identical
        # to the two launches below)
        lattice, lh, lw, lpad, _ = lat
        tiles, bias2 = layer2.x3
        enc = torch.empty(S * 3, C // 2, **f32)
        if eng._ran(lib.car_lattice_encode_linear, _ptr(lattice), lh, lw, lpad, _ptr(src), _ptr(rgrid), _ptr(rpe), _ptr(wpt), n, S * 3,
                    _ptr(tiles), _ptr(bias2), C, C // 2, _ptr(enc), C // 2, 0, _stream()):
            return enc.view(S, 3 * (C // 2))
        eng.fuse_exchange = False
    h1 = torch.empty(S * 3, C, **f32)
    if lat is not None:                                     # four taps of the merged lattice per row instead of twelve
        lattice, lh, lw, lpad, _ = lat
        lib.car_lattice_encode_rows(_ptr(lattice), lh, lw, lpad, C, _ptr(src), _ptr(rgrid), _ptr(rpe), _ptr(wpt), n, S * 3, _ptr(h1), C, _stream())
    else:
        lib.car_gather_encode_rows(ptrs, hs, ws, L, C, _ptr(src), _ptr(rgrid), _ptr(rpe), _ptr(wpt), n, S * 3, _ptr(h1), C, _stream())
    enc = torch.empty(S * 3, C // 2, **f32)
    eng.linear(h1, C, layer2, enc, C // 2, S * 3)
    return enc.view(S, 3 * (C // 2))                          # component-major: the consumers' weights are permuted (_weights)


def _keys_and_queries(r: _Run, e: Tensor, g: Tensor):
    """a12: keys;  a13: geometric query.  The value projection (latent_value, no nonlinearity before the weighted sum)
    commutes with the attention average: sum_s w_s (Wv e_s + bv) = Wv (sum_s w_s e_s) + bv because the softmax
    weights of a ray sum to 1, so it is applied once per ray after the reduction instead of once per sample.
    -> q, and the keys or (car_key_query_logits) the first round's logits, the other None."""
    eng, pk, S, Ce, f32 = r.eng, r.pk, r.S, r.Ce, r.f32
    keep = r.save is not None
    kmap = pk["key_map.kmajor" if r.kmajor else "key_map"]
    q = torch.empty(S, 128, **f32)
    key = logit1 = None
    if (not keep and eng.fuse_kq and eng.linear_x3 and not eng.linear_flags and kmap.x3 is not None and kmap.N == 128 and eng.m.hidden_dim == 128
            and Ce % 4 == 0 and e.data_ptr() % 16 == 0 and S >= eng.linear_x3_min_rows):
        # key_map -> relu -> key_map_2, query_embed -> relu -> query_embed_2 and the first round's logits in one kernel: the 128-wide
        # k1 / key / q1 rows are never written (csrc/car_linear16.hip, KQ instance)
        tiles, bias_k1 = kmap.x3
        tail, tail_bias = eng._kq_weights(e.device)
        logit1 = torch.empty(S, **f32)
        if not eng._ran(eng.lib.car_key_query_logits, _ptr(e), Ce, _ptr(tiles), _ptr(bias_k1), Ce, _ptr(g), _ptr(tail), _ptr(tail_bias), S, _ptr(q),
                        _ptr(logit1), r.st):
            eng.fuse_kq, logit1 = False, None                      # LDS reservation refused: the five separate launches below
    if logit1 is None:
        k1 = torch.empty(S, 128, **f32)
        eng.linear(e, Ce, kmap, k1, 128, S, RELU_OUT)
        key = torch.empty(S, 128, **f32)
        eng.linear(k1, 128, pk["key_map_2"], key, 128, S)
        q1 = torch.empty(S, 128, **f32) if keep else k1             # inference: the query's hidden layer in k1's buffer
        eng.linear(g, 16, pk["query_embed"], q1, 128, S, RELU_OUT)
        eng.linear(q1, 128, pk["query_embed_2"], q, 128, S)
        if keep:
            r.save.k1, r.save.key, r.save.q1, r.save.q = k1, key, q1, q
    return q, key, logit1


def _attention_rounds(r: _Run, e: Tensor, g: Tensor, q: Tensor, key: Optional[Tensor], logit1: Optional[Tensor], pt: Tensor):
    """a14 + a16: attention round 1, depth read-out;  a15: the second round.  -> at_wt, at_wt2 (None without repeat_attention), depth,
    at_wt_max and the latent z replicated per view [bR, V Dl]."""
    eng, lib, m, pk, sv, st, f32 = r.eng, r.eng.lib, r.eng.m, r.pk, r.save, r.st, r.f32
    b, V, R, P, n, S, bR, Ce, Dl = r.b, r.V, r.R, r.P, r.n, r.S, r.bR, r.Ce, r.eng.m.latent_dim
    keep = sv is not None
    at_wt = torch.empty(n, R, P, **f32)
    depth = torch.empty(b, R, 1, **f32)
    amax = torch.empty(n, R, 1, dtype=torch.int32, device=e.device)
    ebar1 = torch.empty(bR, Ce, **f32)
    lg, qr = (logit1, None) if logit1 is not None else (key, q)    # the logits of car_key_query_logits, or keys and queries
    lib.car_attend(_ptr(lg), _ptr(qr), 128, _ptr(e), Ce, b, V, R, P, None, 0.0, _ptr(at_wt), _ptr(ebar1), Ce, 1, _ptr(pt), _ptr(r.poses), _ptr(depth),
                   _ptr(amax), st)
    lv = pk["latent_value.kmajor" if r.kmajor else "latent_value"]
    zrep = torch.empty(bR, V * Dl, **f32)
    at_wt2 = None
    if m.repeat_attention:
        z1 = torch.empty(bR, Dl, **f32)
        eng.linear(ebar1, Ce, lv, z1, Dl, bR)
        # a15: second round; the z_embed half of query_repeat_embed is per ray, the local_coords half per sample
        hb = torch.empty(bR, 128, **f32)
        eng.linear(z1, Dl, pk["encode_latent"], hb, 128, bR)
        uh = torch.empty(bR, 128, **f32)
        eng.linear(hb, 128, pk["query_repeat_embed.h"], uh, 128, bR)
        at_wt2 = torch.empty(n, R, P, **f32)
        ebar2 = torch.empty(bR, Ce, **f32) if keep else ebar1      # inference: round 2's average in round 1's buffer
        if eng.fuse_round2 and not keep:
            # ug = Wr1[:,128:] g + br1, q2 = Wr2 relu(ug + uh) + b and <q2, qry>/16 in one kernel: neither is written
            r2w, r2b = eng._round2_weights(e.device)
            logit2 = torch.empty(S, **f32)
            lib.car_round2_logits(_ptr(g), _ptr(uh), _ptr(q), _ptr(r2w), _ptr(r2b), b, V, R, P, _ptr(logit2), st)
            lib.car_attend(_ptr(logit2), None, 128, _ptr(e), Ce, b, V, R, P, None, 0.0, _ptr(at_wt2), _ptr(ebar2), Ce, 1, None, None, None, None, st)
        else:
            k1r = torch.empty(S, 128, **f32)
            eng.linear(g, 16, pk["query_repeat_embed.g"], k1r, 128, S)
            lib.car_add_ray_bias_relu(_ptr(k1r), _ptr(uh), b, V, R, P, 128, st)
            key2 = torch.empty(S, 128, **f32) if keep or key is None else key   # inference: round 2's keys in round 1's buffer
            eng.linear(k1r, 128, pk["query_repeat_embed_2"], key2, 128, S)
            lib.car_attend(_ptr(key2), _ptr(q), 128, _ptr(e), Ce, b, V, R, P, None, 0.0, _ptr(at_wt2), _ptr(ebar2), Ce, 1, None, None, None, None, st)
            if keep:
                sv.k1r, sv.key2 = k1r, key2
        # z = (Wv ebar2 + bv) + V * z1   (models.py:561-565: "+ z_local" per view, then the view sum)
        if keep:
            lib.car_add(_ptr(zrep), V * Dl, _ptr(z1), Dl, float(V), None, 0, 0.0, bR, Dl, st)
            sv.z1, sv.hb, sv.at_wt2, sv.ebar2 = z1, hb, at_wt2, ebar2
        else:
            zrep.view(bR, V, Dl)[:, 0] = z1 * float(V)
        eng.linear(ebar2, Ce, lv, zrep, V * Dl, bR, ACCUM)
    else:
        eng.linear(ebar1, Ce, lv, zrep, V * Dl, bR)
    # the per-view replication of models.py:541, 565, 605-606
    if keep:
        for v in range(1, V):
            lib.car_add(_ptr(zrep[:, v * Dl:]), V * Dl, _ptr(zrep), V * Dl, 1.0, None, 0, 0.0, bR, Dl, st)
        sv.at_wt, sv.ebar1, sv.zrep = at_wt, ebar1, zrep
    elif V > 1:
        zv = zrep.view(bR, V, Dl)
        zv[:, 1:] = zv[:, :1]
    return at_wt, at_wt2, depth, amax, zrep


def _decode(r: _Run, phi_x: Tensor, ld_phi: int, zrep: Tensor, rays: Tensor):
    """a17: light-field decoder;  a18: valid mask, white background.  -> rgb, valid."""
    eng, m, pk, sv, f32 = r.eng, r.eng.m, r.pk, r.save, r.f32
    b, V, R, bR, Dl, hid = r.b, r.V, r.R, r.bR, r.eng.m.latent_dim, r.eng.m.phi.d_hidden
    keep = sv is not None
    x = torch.empty(bR, hid, **f32)
    net = None if keep else torch.empty(bR, hid, **f32)
    eng.linear(phi_x, ld_phi, pk["phi.lin_in"], x, hid, bR)
    xas, nets = [], []
    for i in range(m.phi.n_blocks):
        if keep:                                                   # the backward reads every block's input and hidden activation
            x, net = x.clone(), torch.empty(bR, hid, **f32)
            xas.append(x)
            nets.append(net)
        eng.linear(zrep, V * Dl, pk[f"phi.lin_z.{i}"], x, hid, bR, ACCUM)
        eng.linear(x, hid, pk[f"phi.blocks.{i}.fc_0"], net, hid, bR, RELU_IN)
        if keep:
            x = x.clone()
        eng.linear(net, hid, pk[f"phi.blocks.{i}.fc_1"], x, hid, bR, RELU_IN | ACCUM)
    out3 = torch.empty(bR, 4, **f32)
    eng.linear(x, hid, pk["phi.lin_out"], out3, 4, bR, RELU_IN)
    rgb = torch.empty(b, 1, R, 3, **f32)
    valid = torch.empty(b, R, 1, **f32)
    eng.lib.car_finalize(_ptr(rays), _ptr(out3), 4, b, V, R, _ptr(rgb), _ptr(valid), r.st)
    if keep:
        sv.phi_x, sv.xas, sv.nets, sv.dec_out, sv.valid = phi_x, xas, nets, x, valid
    return rgb, valid
