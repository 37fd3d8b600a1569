"""Training-side entry of the render path: the forward of the staged route with every intermediate kept, its
backward, and the gradient all-reduce of the reference's training loop.

The reference trains with torch autograd over ``CrossAttentionRenderer.forward`` (training.py:92-136): ``model(model_input)`` on a few
hundred random rays per scene, a loss on ``rgb`` (and optionally ``depth_ray``, loss_functions.py:74-132), ``backward()``, then
``average_gradients`` (training.py:21-28) when several GPUs train replicas.  Here ``render_train`` is that forward as a
``torch.autograd.Function`` whose forward AND backward are HIP kernels of ``libcar_hip.so``:

  forward   the staged forward (``staged.forward``) with a ``staged.Saved`` record: its literal stage forms (gather -> 579-wide GEMM,
            five key / query launches, the unfused second round), none fused away, because the backward needs what the fused
            inference kernels never write: the gathered rows, the first layer's activations, keys, queries;
  backward  ``car_linear`` with transposed weights (data gradients), ``car_linear_wgrad`` (weight / bias gradients),
            ``car_attend_backward``, ``car_gather_bilinear_backward`` (scatter-add into the pyramid), and the element-wise pieces
            (csrc/car_backward.hip) — sequenced as the forward is: one function per stage of staged.py, named after it
            (``_decode_backward`` ... ``_scatter_to_pyramid``), called last to first over one run record (``_Run``); what "the
            backward of a linear layer" is stands once, in ``_linear_backward``.

Gradients flow to every renderer parameter on the path and to the feature pyramid ``z`` — and through ``z``, by ordinary torch
autograd, into the encoder when ``z`` came from ``get_z``.  The geometry is not differentiated: nothing in it depends on a parameter.
PyTorch is plumbing here as everywhere: storage, views, the autograd graph edge, ``torch.distributed``.

Supported: every constructor variant of the reference — the default cross-view exchange (``n_view=2``), the three-view exchange
(``n_view=3``, models.py:345-475), the single-view merge layer (``n_view=1``, models.py:478-485), ``no_latent_concat`` (the gathered
features go straight into the attention, models.py:476-477), epipolar or depth sampling (``no_sample``), with or without the second
attention round, any channel widths.
"""
from __future__ import annotations

import collections
import ctypes
from typing import Dict, List, Optional

import torch

from . import staged
from .engine import (ACCUM, PLACE_OTHER2, PLACE_OWN, PLACE_PLAIN, RELU_IN, WGRAD_FP32, PackedLinear, RenderEngine, _Cached, _levels, _mode, _ptr,
                     _render_layers, _round_up, _stream)

Tensor = torch.Tensor


class _Ops:
    """What the backward keeps on the engine from step to step (``eng._train_ops``) — the transposed weights, re-packed only when the
    optimizer changed them — beside the entry points whose arguments need marshalling: the weight gradient's flags, the scatters' level
    and gather tables.  Every other entry is called on the checked handle directly, as in staged.py."""

    def __init__(self, eng: RenderEngine):
        self.eng, self.lib = eng, eng.lib
        self._t: Dict[str, _Cached] = collections.defaultdict(_Cached)

    def transposed(self, name: str, w: Tensor) -> PackedLinear:
        """W [N, K] -> the layer x -> x W (weight W^T [K, N], no bias): car_linear then computes dX = dY W."""
        return self._t[name].get([w], (), lambda: PackedLinear(w.detach().reshape(w.shape[0], -1).t().contiguous(), None, w.device, name + "^T"))

    def wgrad(self, dy: Tensor, ldy: int, x: Tensor, ldx: int, M: int, N: int, K: int, dw: Tensor, lddw: int, db: Optional[Tensor], relu_x=False):
        # engine.wgrad_fp32 = True keeps the wide layers' weight gradients on the fp32 matrix pipe (CAR_WGRAD_FP32): the reference's fp32
        # arithmetic term for term, at half the rate of the default bf16 hi / lo x 3 kernel (~2^-17 per term)
        flags = (RELU_IN if relu_x else 0) | (WGRAD_FP32 if self.eng.wgrad_fp32 else 0)
        self.lib.car_linear_wgrad(_ptr(dy), ldy, _ptr(x), ldx, M, N, K, flags, _ptr(dw), lddw, _ptr(db), _stream())

    def gather_backward(self, dmaps: List[Tensor], grid: Tensor, pts: int, mode: int, place: int, V: int, dout: Tensor, ld_out: int, col_out: int):
        ptrs, cs, hs, ws, L = _levels(dmaps)
        self.lib.car_gather_bilinear_backward(ptrs, cs, hs, ws, L, dmaps[0].shape[0], _ptr(grid), pts, mode, place, V, _ptr(dout), ld_out,
                                              col_out, _stream())

    def gather_backward_binned(self, maps: List[Tensor], gathers, pts: int, V: int, dout: Tensor, ld_out: int, col_out: int) -> List[Tensor]:
        """The gradient of the gathered rows `dout` with respect to `maps` for all `gathers` [(grid, padding mode, placement)] at once, every
        texel written exactly once (csrc/car_scatter.hip: taps binned by texel, no floating-point atomics, no zero fill)."""
        G = len(gathers)
        dmaps = [torch.empty_like(m) for m in maps]
        ptrs, cs, hs, ws, L = _levels(dmaps)
        grids = (ctypes.c_void_p * G)(*[g[0].data_ptr() for g in gathers])
        modes = (ctypes.c_int * G)(*[g[1] for g in gathers])
        places = (ctypes.c_int * G)(*[g[2] for g in gathers])
        n_maps = maps[0].shape[0]
        nbytes = self.lib.car_scatter_workspace_bytes(hs, ws, L, n_maps, pts, G)
        work = torch.empty(nbytes, dtype=torch.uint8, device=dout.device)
        self.lib.car_gather_bilinear_backward_binned(ptrs, cs, hs, ws, L, n_maps, grids, modes, places, G, pts, V, _ptr(dout), ld_out, col_out,
                                                     _ptr(work), nbytes, _stream())
        return dmaps


# parameters the path reads, in the order their gradients are returned
def _param_names(m) -> List[str]:
    layers = _render_layers(m)
    names = layers.head + layers.attention + (layers.round2 if m.repeat_attention else []) + layers.decoder
    return [n + k for n in names for k in (".weight", ".bias")]


# What the stages of one backward share, in the manner of staged._Run: the engine, the checked handle, the engine's _Ops, the forward's
# record, engine._mode, the sizes (n = b V maps, S = b V R P samples, bR = b R rays, C the pyramid's channels, Ce the width of e,
# Dl = latent_dim, hid the decoder's width, the row strides of enc_rows and phi_x), the parameters by name and the views of the flat
# buffer their gradients are summed into, the tensor options, whether the pyramid asked for a gradient, (dtype, asked, lies channel-last)
# per pyramid level, and the launch stream.
_Run = collections.namedtuple("_Run", "eng lib ops sv mode b V R P n S bR C Ce Dl hid ld_rows ld_phi par grads f32 need_dz levels st")


def _start(ctx) -> _Run:
    """The run record of one backward.  The sizes come from the record and the module; the first allocation is the one zero fill for all
    parameter gradients (views of a flat buffer, 16-byte aligned), not one per tensor."""
    sv, m, par = ctx.saved, ctx.module, ctx.params
    eng: RenderEngine = m._engine
    ops = getattr(eng, "_train_ops", None)                  # kept on the engine: its transposed-weight cache (engine._Cached per layer)
    if ops is None or ops.eng is not eng:                   # then survives from step to step and re-packs only what the optimizer changed
        ops = eng._train_ops = _Ops(eng)
    (b, R), P = sv.valid.shape[:2], m.npoints
    V = sv.pixel_val.shape[0] // b
    f32 = dict(device=sv.e.device, dtype=torch.float32)
    sizes = {k: v.numel() for k, v in par.items()}
    flat = torch.zeros(sum(_round_up(n, 4) for n in sizes.values()), **f32)
    grads: Dict[str, Tensor] = {}
    at = 0
    for k, v in par.items():
        grads[k] = flat[at:at + sizes[k]].view(v.shape)
        at += _round_up(sizes[k], 4)
    return _Run(eng=eng, lib=eng.lib, ops=ops, sv=sv, mode=_mode(m), b=b, V=V, R=R, P=P, n=b * V, S=b * V * R * P, bR=b * R,
                C=sum(t.shape[3] for t in sv.maps), Ce=sv.Ce, Dl=m.latent_dim, hid=m.phi.d_hidden, ld_rows=sv.ld_rows, ld_phi=sv.ld_phi, par=par,
                grads=grads, f32=f32, need_dz=ctx.need_dz, levels=list(zip(ctx.z_dtypes, ctx.needs_input_grad[3:3 + ctx.n_levels], ctx.z_channel_last)),
                st=_stream())


def _wgrad(r: _Run, name: str, dy: Tensor, ldy: int, x: Tensor, ldx: int, M: int, relu_x=False, col0=0, K=None, bias=True) -> None:
    """car_linear_wgrad of layer ``name`` into its gradient views: dW[:, col0:col0 + K] += dy^T x (``relu_x``: dy^T relu(x)) over M rows and,
    unless ``bias=False``, db += the column sums of dy.  K = None: every column."""
    w = r.grads[name + ".weight"]
    N, Kfull = w.shape[0], w[0].numel()
    r.ops.wgrad(dy, ldy, x, ldx, M, N, Kfull if K is None else K, w.view(N, Kfull)[:, col0:], Kfull, r.grads[name + ".bias"] if bias else None, relu_x)


def _linear_backward(r: _Run, name: str, dy: Tensor, ldy: int, x: Tensor, ldx: int, M: int, relu_x=False, out: Optional[Tensor] = None, ldo=0,
                     flags=0, cols: Optional[int] = None, relu=None) -> None:
    """The backward of the linear layer ``name`` (y = W x + b over M rows): its weight and bias gradients (_wgrad), then, when ``out`` is
    given, its data gradient out = dy W (``ACCUM`` in ``flags``: out += dy W) through engine.linear with the cached transposed weight.
    ``cols``: only the first ``cols`` input columns get a gradient (the rest — point coordinates — never need one): the transposed layer
    then has a multiple of 32 outputs and runs on the split-fp16 path (engine.linear).
    ``relu = (act, lda)``: the layer's input was relu(act) — the gradient is zeroed where act <= 0 as it is stored."""
    _wgrad(r, name, dy, ldy, x, ldx, M, relu_x)
    if out is not None:
        w = r.par[name + ".weight"]
        if cols is not None:
            w, name = w.reshape(w.shape[0], -1)[:, :cols], f"{name}[:, :{cols}]"
        r.eng.linear(dy, ldy, r.ops.transposed(name, w), out, ldo, M, flags, mask=relu)


def _decode_backward(r: _Run, d_rgb: Optional[Tensor]) -> Tensor:
    """Adjoint of staged._decode (a18 / a17): the white background's scaling by ``valid``, phi.lin_out, the blocks last to first,
    phi.lin_in, and the sum of the V copies of z.  -> d z [bR, Dl]."""
    lib, sv, st, f32 = r.lib, r.sv, r.st, r.f32
    b, V, R, bR, Dl, hid = r.b, r.V, r.R, r.bR, r.Dl, r.hid
    d_rgb = torch.zeros(b, R, 3, **f32) if d_rgb is None else d_rgb.detach().reshape(b, R, 3).float().contiguous()
    d_out3 = torch.zeros(bR, 4, **f32)
    lib.car_scale_rows(_ptr(d_out3), 4, _ptr(d_rgb), 3, _ptr(sv.valid), 1, 1.0, bR, 3, 0, st)
    d_x = torch.empty(bR, hid, **f32)
    _linear_backward(r, "phi.lin_out", d_out3, 4, sv.dec_out, hid, bR, relu_x=True, out=d_x, ldo=hid, relu=(sv.dec_out, hid))
    d_zrep = torch.zeros(bR, V * Dl, **f32)
    d_net = torch.empty(bR, hid, **f32)
    tmp = torch.empty(bR, hid, **f32)
    for (lin_z, fc_0, fc_1), xa, net in reversed(list(zip(_render_layers(r.eng.m).blocks, sv.xas, sv.nets))):
        _linear_backward(r, fc_1, d_x, hid, net, hid, bR, relu_x=True, out=d_net, ldo=hid, relu=(net, hid))
        _linear_backward(r, fc_0, d_net, hid, xa, hid, bR, relu_x=True, out=tmp, ldo=hid, relu=(xa, hid))
        lib.car_add(_ptr(d_x), hid, _ptr(d_x), hid, 1.0, _ptr(tmp), hid, 1.0, bR, hid, st)        # d xa = d x + (d net Wfc0) [xa > 0]
        _linear_backward(r, lin_z, d_x, hid, sv.zrep, V * Dl, bR, out=d_zrep, ldo=V * Dl, flags=ACCUM)
    _wgrad(r, "phi.lin_in", d_x, hid, sv.phi_x, r.ld_phi, bR)           # no pair: the ray coordinates phi_x take no gradient
    # the V copies of z
    d_z = torch.empty(bR, Dl, **f32)
    if V == 1:
        lib.car_add(_ptr(d_z), Dl, _ptr(d_zrep), V * Dl, 1.0, None, 0, 0.0, bR, Dl, st)
    else:
        lib.car_add(_ptr(d_z), Dl, _ptr(d_zrep), V * Dl, 1.0, _ptr(d_zrep[:, Dl:]), V * Dl, 1.0, bR, Dl, st)
    for v in range(2, V):
        lib.car_add(_ptr(d_z), Dl, _ptr(d_z), Dl, 1.0, _ptr(d_zrep[:, v * Dl:]), V * Dl, 1.0, bR, Dl, st)
    return d_z


def _attention_rounds_backward(r: _Run, d_z: Tensor, d_depth: Optional[Tensor]):
    """Adjoint of staged._attention_rounds: a15 (the second round: latent_value over ebar2, its attention, the query_repeat_embed /
    encode_latent chain back to z1), then a14 / a16 (latent_value over ebar1, the first round's attention with the depth read-out's
    cotangent).  -> d e [S, Ce] (both rounds' value terms) and, for the keys' and queries' layers, d key [S, 128] and d q [S, 128]."""
    lib, sv, st, f32 = r.lib, r.sv, r.st, r.f32
    b, V, R, P, S, bR, Ce, Dl = r.b, r.V, r.R, r.P, r.S, r.bR, r.Ce, r.Dl
    repeat = r.eng.m.repeat_attention
    d_e = torch.empty(S, Ce, **f32)
    d_q = torch.empty(S, 128, **f32)
    d_key = torch.empty(S, 128, **f32)                         # round 2's d key2 first, then round 1's d key
    dlogit = torch.empty(S, **f32)                             # either round's
    d_ebar = torch.empty(bR, Ce, **f32)                        # either round's
    d_depth = None if d_depth is None else d_depth.detach().reshape(bR).float().contiguous()
    if repeat:
        # ---- a15: z = V z1 + latent_value(ebar2)
        _linear_backward(r, "latent_value", d_z, Dl, sv.ebar2, Ce, bR, out=d_ebar, ldo=Ce)
        lib.car_attend_backward(_ptr(sv.at_wt2), _ptr(sv.e), Ce, b, V, R, P, _ptr(d_ebar), Ce, None, None, None, _ptr(d_e), 0, _ptr(dlogit), st)
        lib.car_scale_rows(_ptr(d_key), 128, _ptr(sv.q), 128, _ptr(dlogit), 1, 1.0 / 16.0, S, 128, 0, st)              # d key2
        lib.car_scale_rows(_ptr(d_q), 128, _ptr(sv.key2), 128, _ptr(dlogit), 1, 1.0 / 16.0, S, 128, 0, st)
        d_k1r = torch.empty(S, 128, **f32)
        _linear_backward(r, "query_repeat_embed_2", d_key, 128, sv.k1r, 128, S, out=d_k1r, ldo=128, relu=(sv.k1r, 128))
        # no pair: query_repeat_embed ran as two layers (staged._attention_rounds) — its local_coords half per sample, which takes the
        # bias and no data gradient, and its z_embed half per ray, over the sum of a ray's samples
        _wgrad(r, "query_repeat_embed", d_k1r, 128, sv.g, 16, S, col0=128, K=16)
        d_uh = torch.empty(bR, 128, **f32)
        lib.car_reduce_samples(_ptr(d_k1r), b, V, R, P, 128, _ptr(d_uh), st)
        _wgrad(r, "query_repeat_embed", d_uh, 128, sv.hb, 128, bR, col0=0, K=128, bias=False)
        d_hb = torch.empty(bR, 128, **f32)
        w_h = r.par["query_repeat_embed.weight"].reshape(128, -1)[:, :128]
        r.eng.linear(d_uh, 128, r.ops.transposed("query_repeat_embed.h", w_h), d_hb, 128, bR)
        # no pair: d z1 = V d z, written between encode_latent's two calls, + d hb W
        _wgrad(r, "encode_latent", d_hb, 128, sv.z1, Dl, bR)
        d_z1 = torch.empty(bR, Dl, **f32)
        lib.car_add(_ptr(d_z1), Dl, _ptr(d_z), Dl, float(V), None, 0, 0.0, bR, Dl, st)
        r.eng.linear(d_hb, 128, r.ops.transposed("encode_latent", r.par["encode_latent.weight"]), d_z1, Dl, bR, ACCUM)
        d_z = d_z1
    # ---- a14 / a16: z1 (or z) = latent_value(ebar1); depth read-out
    _linear_backward(r, "latent_value", d_z, Dl, sv.ebar1, Ce, bR, out=d_ebar, ldo=Ce)
    lib.car_attend_backward(_ptr(sv.at_wt), _ptr(sv.e), Ce, b, V, R, P, _ptr(d_ebar), Ce, _ptr(d_depth), _ptr(sv.pt), _ptr(sv.poses), _ptr(d_e),
                            int(repeat), _ptr(dlogit), st)
    lib.car_scale_rows(_ptr(d_key), 128, _ptr(sv.q), 128, _ptr(dlogit), 1, 1.0 / 16.0, S, 128, 0, st)
    lib.car_scale_rows(_ptr(d_q), 128, _ptr(sv.key), 128, _ptr(dlogit), 1, 1.0 / 16.0, S, 128, int(repeat), st)
    return d_e, d_key, d_q


def _keys_and_queries_backward(r: _Run, d_e: Tensor, d_key: Tensor, d_q: Tensor) -> None:
    """Adjoint of staged._keys_and_queries (a12, a13): key_map_2 and key_map, whose data gradient is added to d e; query_embed_2 and
    query_embed."""
    sv, S = r.sv, r.S
    d_k1 = torch.empty(S, 128, **r.f32)
    _linear_backward(r, "key_map_2", d_key, 128, sv.k1, 128, S, out=d_k1, ldo=128, relu=(sv.k1, 128))
    _linear_backward(r, "key_map", d_k1, 128, sv.e, r.Ce, S, out=d_e, ldo=r.Ce, flags=ACCUM)
    _linear_backward(r, "query_embed_2", d_q, 128, sv.q1, 128, S, out=d_k1, ldo=128, relu=(sv.q1, 128))      # d q1, in d k1's buffer
    _wgrad(r, "query_embed", d_k1, 128, sv.g, 16, S)                   # no pair: the local coordinates g take no gradient


# ---------------------------------------------------------------------- adjoints of the per-sample features e, one function per mode:
# -> (gradient of the gathered rows, its row stride, [(grid, padding mode, placement)]) for _scatter_to_pyramid, None when the pyramid
# asked for no gradient; the three-view exchange scatters for itself and returns the levels' gradients
def _point_mlp_backward(r: _Run, d_enc: Tensor, M: int) -> Optional[Tensor]:
    """a11 backwards over M rows, what the two- and the three-view route share: query_encode_latent_2, then query_encode_latent, whose data
    gradient — the first C columns of the input rows [M, ld_rows] — is taken and returned only when the pyramid asked for one (z from get_z
    under autograd, or a leaf)."""
    sv, C, ld = r.sv, r.C, r.ld_rows
    d_h1 = torch.empty(M, C, **r.f32)
    _linear_backward(r, "query_encode_latent_2", d_enc, C // 2, sv.h1, C, M, out=d_h1, ldo=C, relu=(sv.h1, C))
    d_rows = torch.empty(M, ld, **r.f32) if r.need_dz else None
    _linear_backward(r, "query_encode_latent", d_h1, C, sv.enc_rows, ld, M, out=d_rows, ldo=ld, cols=C)
    return d_rows


def _e_concat2_backward(r: _Run, d_e: Tensor):
    """Adjoint of staged._e_concat2's training form."""
    d_rows = _point_mlp_backward(r, d_e, r.S * r.V)
    return None if d_rows is None else (d_rows, r.ld_rows, [(r.sv.pixel_val, 0, PLACE_OWN), (r.sv.grid_other, 1, PLACE_OTHER2)])


def _encode_three_views_backward(r: _Run, d_e: Tensor) -> Optional[list]:
    """Adjoint of staged._encode_three_views' training form: its own scatter, one atomic launch per gather."""
    sv, b, V, S, C, ld, pts = r.sv, r.b, r.V, r.S, r.C, r.ld_rows, r.R * r.P
    # e[s, ch * 3 + k] = enc[(s, k), ch] (models.py:446): back to one row per (sample, component)
    d_enc = d_e.view(S, C // 2, 3).permute(0, 2, 1).contiguous().view(S * 3, C // 2)
    d_rows = _point_mlp_backward(r, d_enc, S * 3)
    if d_rows is None:
        return None
    d_rv = d_rows.view(b, V, pts, 3, ld)
    dmaps = [torch.zeros_like(t) for t in sv.maps]
    d_own = d_rv[:, :, :, 0, :C].contiguous().view(S, C)              # component 0: the view's own features at its own samples
    r.ops.gather_backward(dmaps, sv.pixel_val, pts, 0, PLACE_PLAIN, V, d_own, C, 0)
    for c_, o_, k_, grid in sv.cross:                                 # component k of context c: view o's features at `grid`
        d_cross = d_rv[:, c_, :, k_, :C].contiguous().view(b * pts, C)
        dm_o = [torch.zeros(b, *t.shape[1:], **r.f32) for t in sv.maps]
        r.ops.gather_backward(dm_o, grid, pts, 1, PLACE_PLAIN, 1, d_cross, C, 0)
        for full, part in zip(dmaps, dm_o):
            full.view(b, V, *full.shape[1:])[:, o_] += part
    return _level_grads(r, dmaps)


def _e_single_backward(r: _Run, d_e: Tensor):
    """Adjoint of staged._e_single."""
    d_rows = torch.empty(r.S, r.ld_rows, **r.f32) if r.need_dz else None
    _linear_backward(r, "update_val_merge", d_e, r.Ce, r.sv.enc_rows, r.ld_rows, r.S, out=d_rows, ldo=r.ld_rows, cols=r.C)
    return None if d_rows is None else (d_rows, r.ld_rows, [(r.sv.pixel_val, 0, PLACE_PLAIN)])


def _e_plain_backward(r: _Run, d_e: Tensor):
    """Adjoint of staged._e_plain: the gathered features are e."""
    return (d_e, r.Ce, [(r.sv.pixel_val, 0, PLACE_PLAIN)]) if r.need_dz else None


def _scatter_to_pyramid(r: _Run, d_rows: Tensor, ld: int, gathers: list) -> list:
    """Adjoint of the gathers (a7 / a10): the gathered rows' gradient into the pyramid — taps binned by texel, every texel written once
    (engine.scatter_atomics = True: the fp32-atomic scatter, one launch per gather into zeroed maps; A/B and tests)."""
    pts = r.R * r.P
    if r.eng.scatter_atomics:
        dmaps = [torch.zeros_like(t) for t in r.sv.maps]
        for grid, pad_mode, place in gathers:
            r.ops.gather_backward(dmaps, grid, pts, pad_mode, place, r.V, d_rows, ld, 0)
    else:
        dmaps = r.ops.gather_backward_binned(r.sv.maps, gathers, pts, r.V, d_rows, ld, 0)
    return _level_grads(r, dmaps)


def _level_grads(r: _Run, dmaps: List[Tensor]) -> list:
    """The channel-last scatter buffers ``dmaps`` as the gradients of the pyramid's levels ([n, C, H, W], the level's dtype); None for
    a level that asked for none."""
    return [(t.permute(0, 3, 1, 2) if cl else t.permute(0, 3, 1, 2).contiguous().to(dt)) if nd else None
            for t, (dt, nd, cl) in zip(dmaps, r.levels)]


class _RenderTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module, inp, n_levels, *tensors):
        z = list(tensors[:n_levels])
        eng: RenderEngine = module._engine
        saved = staged.Saved()
        out = staged.forward(eng, inp, z, save=saved)
        # what the backward's stages cannot take from the record or the module (_start)
        ctx.saved, ctx.module, ctx.n_levels = saved, module, n_levels
        ctx.params = {nme: t for nme, t in zip(_param_names(module), tensors[n_levels:])}
        # the activations live as plain attributes (most are views into buffers autograd does not need to track), so autograd's own
        # version check cannot see an in-place parameter update between forward and backward: check it by hand
        ctx.param_versions = {nme: t._version for nme, t in ctx.params.items()}
        ctx.need_dz = any(ctx.needs_input_grad[3:3 + n_levels])
        ctx.z_dtypes = [t.dtype for t in z]
        # a level that lies channel-last in memory gets its gradient back as a view of the channel-last scatter buffer (same strides as the
        # level: no NHWC -> NCHW copy, as the forward took it without the NCHW -> NHWC one)
        ctx.z_channel_last = [t.dtype == torch.float32 and t.permute(0, 2, 3, 1).is_contiguous() for t in z]
        outs = tuple(out[k] for k in ("rgb", "depth_ray", "valid_mask", "at_wt", "at_wt_max", "coords", "pixel_val"))
        ctx.mark_non_differentiable(*outs[2:])
        return outs

    @staticmethod
    def backward(ctx, d_rgb, d_depth, *_unused):
        """The adjoints of staged.forward's stages, last to first."""
        par = ctx.params
        stale = [k for k, t in par.items() if t._version != ctx.param_versions[k]]
        if stale:
            raise RuntimeError(f"render_train: parameters were modified in place between forward and backward ({stale[:3]} ...): the saved "
                               "activations no longer belong to them")
        with torch.cuda.device(ctx.saved.e.device):
            r = _start(ctx)
            d_z = _decode_backward(r, d_rgb)
            d_e, d_key, d_q = _attention_rounds_backward(r, d_z, d_depth)
            d_z = None
            _keys_and_queries_backward(r, d_e, d_key, d_q)
            dz = d_gather = None
            if r.mode == "concat2":
                d_gather = _e_concat2_backward(r, d_e)
            elif r.mode == "concat3":
                dz = _encode_three_views_backward(r, d_e)
            elif r.mode == "single":
                d_gather = _e_single_backward(r, d_e)
            else:
                d_gather = _e_plain_backward(r, d_e)
            if d_gather is not None:
                dz = _scatter_to_pyramid(r, *d_gather)
        if dz is None:                                        # the pyramid asked for no gradient
            dz = [None] * ctx.n_levels
        return (None, None, None, *dz, *[r.grads[k].view_as(par[k]).to(par[k].dtype) for k in par])


def render_train(module, inp, z: Optional[List[Tensor]] = None) -> Dict[str, Tensor]:
    """``model(model_input)`` of the reference's training loop (training.py:92): the render forward with autograd, on the HIP engine.
    ``rgb`` and ``depth_ray`` carry gradients to the renderer's parameters and to ``z`` (``z=None``: ``get_z`` runs under autograd, so
    the encoder trains too)."""
    m = module
    if getattr(m, "render_precision", "fp32") != "fp32":
        raise ValueError(f"render_train: render_precision={m.render_precision!r} is an inference setting; training runs in fp32 "
                         "(set render_precision='fp32')")
    if m.n_view not in (1, 2, 3):
        raise NotImplementedError("render_train covers one, two or three context views (the reference's n_view)")
    dev = inp["query"]["uv"].device
    if dev.type != "cuda":
        raise RuntimeError("render_train runs on the HIP engine only: move the model, the input dict and z to a ROCm device")
    if z is None:
        z = m.get_z(inp)
    elif not hasattr(m, "H"):
        m.H, m.W = inp["context"]["rgb"].shape[2:4]
    if inp["query"]["uv"].shape[1] != 1:
        raise ValueError("one query view per scene (reference models.py:213, 619)")
    if m._engine is None:
        m._engine = RenderEngine(m)
    sd = dict(m.named_parameters())
    params = [sd[k] for k in _param_names(m)]
    with torch.cuda.device(dev):
        rgb, depth, valid, at_wt, amax, coords, pixel_val = _RenderTrain.apply(m, inp, len(z), *z, *params)
    return {"rgb": rgb, "depth_ray": depth, "valid_mask": valid, "at_wt": at_wt, "at_wts": [at_wt], "at_wt_max": amax, "coords": coords,
            "uv": inp["query"]["uv"], "pixel_val": pixel_val, "z": z}


def average_gradients(module, group=None) -> None:
    """The reference's gradient all-reduce (training.py:21-28): every parameter's gradient summed over the ranks and divided by the
    world size — here as ONE flat bucket per dtype over RCCL (xGMI is point-to-point: one large ring all-reduce instead of one
    latency-bound collective per tensor), copied back in place.

    The bucket is laid out over a rank-INVARIANT list — every parameter that requires a gradient, in ``module.parameters()`` order, zeros
    standing in where this rank has none (an unused branch, an encoder-less rank) — so offsets agree on every rank whatever each one
    back-propagated; one extra float per parameter carries "some rank had a gradient".  A parameter without a gradient on ANY rank keeps
    ``grad = None`` (the optimizer skips it, as in the reference); one that had a gradient elsewhere receives the average here too, so
    the replicas stay in step."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    if world == 1:
        return
    by_dtype: Dict[torch.dtype, List[torch.nn.Parameter]] = {}
    for p in module.parameters():
        if p.requires_grad:
            by_dtype.setdefault(p.dtype if p.grad is None else p.grad.dtype, []).append(p)
    for dt, params in by_dtype.items():
        dev = params[0].device
        has = torch.tensor([0.0 if p.grad is None else 1.0 for p in params], device=dev, dtype=dt)
        flat = torch.cat([(torch.zeros(p.numel(), device=dev, dtype=dt) if p.grad is None else p.grad.reshape(-1)) for p in params] + [has])
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
        n_flags = len(params)
        any_rank = (flat[-n_flags:] > 0).tolist()
        flat /= world
        off = 0
        for p, some in zip(params, any_rank):
            g = flat[off:off + p.numel()].view_as(p)
            off += p.numel()
            if p.grad is not None:
                p.grad.copy_(g)
            elif some:
                p.grad = g.clone()


def make_adam(params, lr: float, betas=(0.99, 0.999)):
    """The reference's optimizer (Adam(lr, betas=(0.99, 0.999)), train_realestate10k.py:93) in torch's fused form where the installed torch
    offers it for the parameters' device — the same update in one kernel instead of ten launches per step (3 ms of a 28 ms step) —,
    the plain form otherwise.  The state dict has the same layout either way."""
    params = list(params)
    try:
        return torch.optim.Adam(lr=lr, params=params, betas=betas, fused=True)
    except (RuntimeError, TypeError, ValueError):
        return torch.optim.Adam(lr=lr, params=params, betas=betas)
