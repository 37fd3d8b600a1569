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
            (csrc/car_backward.hip).

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
from .engine import ACCUM, PLACE_OTHER2, PLACE_OWN, PLACE_PLAIN, RELU_IN, PackedLinear, RenderEngine, _Cached, _levels, _mode, _ptr, _round_up, _stream

Tensor = torch.Tensor
WGRAD_FP32 = 16            # CAR_WGRAD_FP32 (include/car_hip.h)


class _Ops:
    """Thin typed wrappers over the backward entry points of the C ABI (include/car_hip.h)."""

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

    def relu_mask(self, grad: Tensor, ldg: int, act: Tensor, lda: int, M: int, N: int):
        self.lib.car_relu_mask(_ptr(grad), ldg, _ptr(act), lda, M, N, _stream())

    def scale_rows(self, out: Tensor, ldo: int, x: Tensor, ldx: int, s: Tensor, group: int, scale: float, M: int, N: int, accumulate=False):
        self.lib.car_scale_rows(_ptr(out), ldo, _ptr(x), ldx, _ptr(s), group, scale, M, N, int(accumulate), _stream())

    def add(self, out: Tensor, ldo: int, a: Tensor, lda: int, alpha: float, b: Optional[Tensor], ldb: int, beta: float, M: int, N: int):
        self.lib.car_add(_ptr(out), ldo, _ptr(a), lda, alpha, _ptr(b), ldb, beta, M, N, _stream())

    def reduce_samples(self, d: Tensor, b: int, V: int, R: int, P: int, C: int, du: Tensor):
        self.lib.car_reduce_samples(_ptr(d), b, V, R, P, C, _ptr(du), _stream())

    def attend_backward(self, w, val, D, b, V, R, P, dz, ld_dz, ddepth, pt, poses, dval, accumulate, dlogit):
        self.lib.car_attend_backward(_ptr(w), _ptr(val), D, b, V, R, P, _ptr(dz), ld_dz, _ptr(ddepth), _ptr(pt), _ptr(poses), _ptr(dval),
                                     int(accumulate), _ptr(dlogit), _stream())

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
    names = {"concat2": ["query_encode_latent", "query_encode_latent_2"], "concat3": ["query_encode_latent", "query_encode_latent_2"],
             "single": ["update_val_merge"], "plain": []}[_mode(m)]
    names = names + ["latent_value", "key_map", "key_map_2", "query_embed", "query_embed_2"]
    if m.repeat_attention:
        names += ["query_repeat_embed", "query_repeat_embed_2", "encode_latent"]
    names += ["phi.lin_in", "phi.lin_out"]
    for i in range(m.phi.n_blocks):
        names += [f"phi.lin_z.{i}", f"phi.blocks.{i}.fc_0", f"phi.blocks.{i}.fc_1"]
    return [n + k for n in names for k in (".weight", ".bias")]


def _level_grads(ctx, dmaps: List[Tensor]) -> list:
    """The channel-last scatter buffers ``dmaps`` as the gradients of the pyramid's levels ([n, C, H, W], the level's dtype); None for
    a level that asked for none."""
    return [(t.permute(0, 3, 1, 2) if cl else t.permute(0, 3, 1, 2).contiguous().to(dt)) if nd else None
            for t, dt, nd, cl in zip(dmaps, ctx.z_dtypes, ctx.needs_input_grad[3:3 + ctx.n_levels], ctx.z_channel_last)]


class _RenderTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module, inp, n_levels, *tensors):
        z = list(tensors[:n_levels])
        eng: RenderEngine = module._engine
        m = module
        saved = staged.Saved()
        out = staged.forward(eng, inp, z, save=saved)
        b, V = inp["context"]["rgb"].shape[:2]
        R = inp["query"]["uv"].shape[2]
        C = sum(t.shape[3] for t in saved.maps)
        ops = getattr(eng, "_train_ops", None)              # kept on the engine: its transposed-weight cache (engine._Cached per layer)
        if ops is None or ops.eng is not eng:               # then survives from step to step and re-packs only what the optimizer changed
            ops = eng._train_ops = _Ops(eng)
        ctx.saved, ctx.ops, ctx.module, ctx.n_levels = saved, ops, module, n_levels
        ctx.dims = (b, V, R, m.npoints, C, m.latent_dim, saved.Ce, m.phi.d_hidden, saved.ld_rows, saved.ld_phi)
        ctx.mode = _mode(m)
        ctx.params = {nme: t for nme, t in zip(_param_names(m), tensors[n_levels:])}
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
        sv, ops, m = ctx.saved, ctx.ops, ctx.module
        eng: RenderEngine = m._engine
        b, V, R, P, C, Dl, Ce, hid, ld1, ld_phi = ctx.dims
        n, S, bR = b * V, b * V * R * P, b * R
        dev = sv.e.device
        f32 = dict(device=dev, dtype=torch.float32)
        par = ctx.params
        stale = [k for k, t in par.items() if t._version != ctx.param_versions[k]]
        if stale:
            raise RuntimeError(f"render_train: parameters were modified in place between forward and backward ({stale[:3]} ...): the saved "
                               "activations no longer belong to them")
        with torch.cuda.device(dev):
            # one zero fill for all parameter gradients (views of a flat buffer, 16-byte aligned), not one per tensor
            sizes = {k: v.numel() for k, v in par.items()}
            flat = torch.zeros(sum(_round_up(n, 4) for n in sizes.values()), **f32)
            grads: Dict[str, Tensor] = {}
            at = 0
            for k, v in par.items():
                grads[k] = flat[at:at + sizes[k]].view(v.shape)
                at += _round_up(sizes[k], 4)

            def W(name):
                return par[name + ".weight"]

            def wgrad(name, dy, ldy, x, ldx, M, relu_x=False, col0=0, K=None, bias=True):
                w = grads[name + ".weight"]
                N, Kfull = w.shape[0], w[0].numel()
                K = Kfull if K is None else K
                ops.wgrad(dy, ldy, x, ldx, M, N, K, w.view(N, Kfull)[:, col0:], Kfull, grads[name + ".bias"] if bias else None, relu_x)

            def dx(name, dy, ldy, out, ldo, M, flags=0, wt=None, cols=None, relu=None):
                # cols: only the first `cols` input columns get a gradient (the rest — point coordinates — never need one): the transposed
                # layer then has a multiple of 32 outputs and runs on the split-fp16 path (engine.linear)
                # relu = (act, lda): the layer's input was relu(act) — the gradient is zeroed where act <= 0 as it is stored
                w = W(name) if wt is None else wt
                if cols is not None:
                    w, name = w.reshape(w.shape[0], -1)[:, :cols], f"{name}[:, :{cols}]"
                eng.linear(dy, ldy, ops.transposed(name, w), out, ldo, M, flags, mask=relu)

            # ---- a18 / a17: white background, decoder
            d_rgb = torch.zeros(b, R, 3, **f32) if d_rgb is None else d_rgb.detach().reshape(b, R, 3).float().contiguous()
            d_out3 = torch.zeros(bR, 4, **f32)
            ops.scale_rows(d_out3, 4, d_rgb, 3, sv.valid, 1, 1.0, bR, 3)
            wgrad("phi.lin_out", d_out3, 4, sv.dec_out, hid, bR, relu_x=True)
            d_x = torch.empty(bR, hid, **f32)
            dx("phi.lin_out", d_out3, 4, d_x, hid, bR, relu=(sv.dec_out, hid))
            d_zrep = torch.zeros(bR, V * Dl, **f32)
            d_net = torch.empty(bR, hid, **f32)
            tmp = torch.empty(bR, hid, **f32)
            for i in reversed(range(m.phi.n_blocks)):
                fc0, fc1, lz = f"phi.blocks.{i}.fc_0", f"phi.blocks.{i}.fc_1", f"phi.lin_z.{i}"
                xa, net = sv.xas[i], sv.nets[i]
                wgrad(fc1, d_x, hid, net, hid, bR, relu_x=True)
                dx(fc1, d_x, hid, d_net, hid, bR, relu=(net, hid))
                wgrad(fc0, d_net, hid, xa, hid, bR, relu_x=True)
                dx(fc0, d_net, hid, tmp, hid, bR, relu=(xa, hid))
                ops.add(d_x, hid, d_x, hid, 1.0, tmp, hid, 1.0, bR, hid)                             # d xa = d x + (d net Wfc0) [xa > 0]
                wgrad(lz, d_x, hid, sv.zrep, V * Dl, bR)
                dx(lz, d_x, hid, d_zrep, V * Dl, bR, ACCUM)
            wgrad("phi.lin_in", d_x, hid, sv.phi_x, ld_phi, bR)
            # the V copies of z
            d_zf = torch.empty(bR, Dl, **f32)
            if V == 1:
                ops.add(d_zf, Dl, d_zrep, V * Dl, 1.0, None, 0, 0.0, bR, Dl)
            else:
                ops.add(d_zf, Dl, d_zrep, V * Dl, 1.0, d_zrep[:, Dl:], V * Dl, 1.0, bR, Dl)
            for v in range(2, V):
                ops.add(d_zf, Dl, d_zf, Dl, 1.0, d_zrep[:, v * Dl:], V * Dl, 1.0, bR, Dl)

            d_e = torch.empty(S, Ce, **f32)
            d_q = torch.empty(S, 128, **f32)
            d_key = torch.empty(S, 128, **f32)
            dlogit = torch.empty(S, **f32)
            d_ebar = torch.empty(bR, Ce, **f32)
            d_depth_t = None if d_depth is None else d_depth.detach().reshape(bR).float().contiguous()
            have_e = False
            if m.repeat_attention:
                # ---- a15: z = V z1 + latent_value(ebar2)
                wgrad("latent_value", d_zf, Dl, sv.ebar2, Ce, bR)
                dx("latent_value", d_zf, Dl, d_ebar, Ce, bR)
                ops.attend_backward(sv.at_wt2, sv.e, Ce, b, V, R, P, d_ebar, Ce, None, None, None, d_e, False, dlogit)
                have_e = True
                ops.scale_rows(d_key, 128, sv.q, 128, dlogit, 1, 1.0 / 16.0, S, 128)               # d key2
                ops.scale_rows(d_q, 128, sv.key2, 128, dlogit, 1, 1.0 / 16.0, S, 128)
                wgrad("query_repeat_embed_2", d_key, 128, sv.k1r, 128, S)
                d_k1r = torch.empty(S, 128, **f32)
                dx("query_repeat_embed_2", d_key, 128, d_k1r, 128, S, relu=(sv.k1r, 128))
                wr = W("query_repeat_embed").reshape(128, -1)
                wgrad("query_repeat_embed", d_k1r, 128, sv.g, 16, S, col0=128, K=16)              # local_coords half + bias
                d_uh = torch.empty(bR, 128, **f32)
                ops.reduce_samples(d_k1r, b, V, R, P, 128, d_uh)
                wgrad("query_repeat_embed", d_uh, 128, sv.hb, 128, bR, col0=0, K=128, bias=False)  # z_embed half
                d_hb = torch.empty(bR, 128, **f32)
                dx("query_repeat_embed.h", d_uh, 128, d_hb, 128, bR, wt=wr[:, :128])
                wgrad("encode_latent", d_hb, 128, sv.z1, Dl, bR)
                d_z1 = torch.empty(bR, Dl, **f32)
                ops.add(d_z1, Dl, d_zf, Dl, float(V), None, 0, 0.0, bR, Dl)
                dx("encode_latent", d_hb, 128, d_z1, Dl, bR, ACCUM)
                d_zf = d_z1
            # ---- a14 / a16: z1 (or z) = latent_value(ebar1); depth read-out
            wgrad("latent_value", d_zf, Dl, sv.ebar1, Ce, bR)
            dx("latent_value", d_zf, Dl, d_ebar, Ce, bR)
            ops.attend_backward(sv.at_wt, sv.e, Ce, b, V, R, P, d_ebar, Ce, d_depth_t, sv.pt, sv.poses, d_e, have_e, dlogit)
            ops.scale_rows(d_key, 128, sv.q, 128, dlogit, 1, 1.0 / 16.0, S, 128)
            ops.scale_rows(d_q, 128, sv.key, 128, dlogit, 1, 1.0 / 16.0, S, 128, accumulate=m.repeat_attention)
            # ---- a12, a13
            wgrad("key_map_2", d_key, 128, sv.k1, 128, S)
            d_k1 = torch.empty(S, 128, **f32)
            dx("key_map_2", d_key, 128, d_k1, 128, S, relu=(sv.k1, 128))
            wgrad("key_map", d_k1, 128, sv.e, Ce, S)
            dx("key_map", d_k1, 128, d_e, Ce, S, ACCUM)
            wgrad("query_embed_2", d_q, 128, sv.q1, 128, S)
            dx("query_embed_2", d_q, 128, d_k1, 128, S, relu=(sv.q1, 128))                        # d q1 (buffer reused)
            wgrad("query_embed", d_k1, 128, sv.g, 16, S)
            dz = [None] * ctx.n_levels
            mode = ctx.mode
            d_gather = None                                   # (gradient of the gathered rows, its row stride, [(grid, padding mode, placement)])
            if mode == "concat2":
                # ---- a11
                wgrad("query_encode_latent_2", d_e, C // 2, sv.h1, C, S * V)
                d_h1 = torch.empty(S * V, C, **f32)
                dx("query_encode_latent_2", d_e, C // 2, d_h1, C, S * V, relu=(sv.h1, C))
                wgrad("query_encode_latent", d_h1, C, sv.enc_rows, ld1, S * V)
                if ctx.need_dz:                               # the pyramid asked for a gradient (z from get_z under autograd, or a leaf)
                    d_x1 = torch.empty(S * V, ld1, **f32)
                    dx("query_encode_latent", d_h1, C, d_x1, ld1, S * V, cols=C)
                    d_gather = (d_x1, ld1, [(sv.pixel_val, 0, PLACE_OWN), (sv.grid_other, 1, PLACE_OTHER2)])
            elif mode == "concat3":
                # e[s, ch * 3 + k] = enc[(s, k), ch] (models.py:446): back to one row per (sample, component)
                d_enc = d_e.view(S, C // 2, 3).permute(0, 2, 1).contiguous().view(S * 3, C // 2)
                wgrad("query_encode_latent_2", d_enc, C // 2, sv.h1, C, S * 3)
                d_h1 = torch.empty(S * 3, C, **f32)
                dx("query_encode_latent_2", d_enc, C // 2, d_h1, C, S * 3, relu=(sv.h1, C))
                wgrad("query_encode_latent", d_h1, C, sv.enc_rows, ld1, S * 3)
                if ctx.need_dz:
                    d_x3 = torch.empty(S * 3, ld1, **f32)
                    dx("query_encode_latent", d_h1, C, d_x3, ld1, S * 3, cols=C)
                    d_x3v = d_x3.view(b, V, R * P, 3, ld1)
                    dmaps = [torch.zeros_like(t) for t in sv.maps]
                    d_own = d_x3v[:, :, :, 0, :C].contiguous().view(S, C)       # component 0: the view's own features at its own samples
                    ops.gather_backward(dmaps, sv.pixel_val, R * P, 0, PLACE_PLAIN, V, d_own, C, 0)
                    for c_, o_, k_, grid in sv.cross:                          # component k of context c: view o's features at `grid`
                        d_rows = d_x3v[:, c_, :, k_, :C].contiguous().view(b * R * P, C)
                        dm_o = [torch.zeros(b, *t.shape[1:], **f32) for t in sv.maps]
                        ops.gather_backward(dm_o, grid, R * P, 1, PLACE_PLAIN, 1, d_rows, C, 0)
                        for full, part in zip(dmaps, dm_o):
                            full.view(b, V, *full.shape[1:])[:, o_] += part
                    dz = _level_grads(ctx, dmaps)
            elif mode == "single":
                wgrad("update_val_merge", d_e, Ce, sv.enc_rows, ld1, S)
                if ctx.need_dz:
                    d_x1 = torch.empty(S, ld1, **f32)
                    dx("update_val_merge", d_e, Ce, d_x1, ld1, S, cols=C)
                    d_gather = (d_x1, ld1, [(sv.pixel_val, 0, PLACE_PLAIN)])
            elif ctx.need_dz:
                d_gather = (d_e, Ce, [(sv.pixel_val, 0, PLACE_PLAIN)])
            if d_gather is not None:
                # ---- a7 / a10: the gathered rows' gradient into the pyramid — taps binned by texel, every texel written once
                # (engine.scatter_atomics = True: the fp32-atomic scatter, one launch per gather into zeroed maps; A/B and tests)
                if eng.scatter_atomics:
                    dmaps = [torch.zeros_like(t) for t in sv.maps]
                    for grid, pad_mode, place in d_gather[2]:
                        ops.gather_backward(dmaps, grid, R * P, pad_mode, place, V, d_gather[0], d_gather[1], 0)
                else:
                    dmaps = ops.gather_backward_binned(sv.maps, d_gather[2], R * P, V, d_gather[0], d_gather[1], 0)
                dz = _level_grads(ctx, dmaps)
        out = [None, None, None] + dz + [grads[k].view_as(par[k]).to(par[k].dtype) for k in _param_names(m)]
        return tuple(out)


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
    import torch
    params = list(params)
    try:
        return torch.optim.Adam(lr=lr, params=params, betas=betas, fused=True)
    except (RuntimeError, TypeError, ValueError):
        return torch.optim.Adam(lr=lr, params=params, betas=betas)
