"""The multi-view DPT-hybrid image encoder behind ``CrossAttentionRenderer.get_z``.

Runs once per stereo pair, outside the per-ray hot loop.  By default it is plain PyTorch-ROCm (MIOpen convolutions, rocBLAS /
``scaled_dot_product_attention`` for the transformer).  The transformer stage alone — the 12 blocks over the concatenated tokens — also
has a route on the library's own kernels (``MultiViewDPTEncoder.vit_route = "device"``: car_vit_blocks, include/car_encoder.h;
opt-in, inference only), and so has what stands in front of it, the ResNetV2 trunk and the token assembly
(``MultiViewDPTEncoder.trunk_route = "device"``: car_trunk_forward and car_vit_tokens, include/car_trunk.h; opt-in, inference only,
independent of the first switch), and so has what stands behind it, the read-out, the re-assembly and the RefineNet fusion
(``MultiViewDPTEncoder.decoder_route = "device"``: car_decoder_forward, include/car_decoder.h; opt-in, inference only, independent of the
other two).  With all three on the device no torch operator is left between the normalised images and ``[path_2, path_1]``
(``CrossAttentionRenderer.encoder_route = "device_full"``, which also normalises the images and runs ``conv_map`` there).  What matters is that a
reference checkpoint loads unchanged (``encoder.*`` keys and shapes are the reference's) and that ``get_z`` produces the reference's
feature pyramid.

What it computes (reference call sites):
  * ``DPTDepthModel.forward(rgb, rel_pose16, nviews)`` (midas/dpt_depth.py:67-89, 94-117): hybrid backbone -> four reassembled
    feature maps -> RefineNet fusion -> ``[path_2 (256 @ H/4), path_1 (256 @ H/2)]``;
  * the backbone (midas/vit.py:124-202, 392-541 with vit_models.py:10-97): ResNetV2-50 stem + stages (3, 4, 9) at strides 4 / 8 /
    16, a 1x1 projection to 768-wide tokens, a class token, the bilinearly resized position embedding and a ``Linear(16, 768)``
    embedding of the view's relative pose added to every token; then the tokens of ALL views of a scene are concatenated into one
    sequence (midas/vit.py:183-186) and run through 12 pre-norm transformer blocks; blocks 8 and 11 are tapped, split back per view
    (midas/vit.py:65-69), the class token is folded in by ``ProjectReadout`` (midas/vit.py:31-42) and the maps are re-assembled;
  * the fusion blocks (midas/blocks.py:231-341).

Third-party arithmetic.  The reference builds the ResNetV2 trunk, the transformer ``Block`` and ``HybridEmbed`` from
``timm==0.5.4`` (requirements.txt; vit_models.py:1-4), which is not part of the reference tree and not installed here.  Those
pieces are restated below from timm 0.5.4's published definitions (``resnetv2.py``: non-pre-activation ``Bottleneck``,
``StdConv2dSame`` weight standardisation with TF "SAME" padding, ``GroupNormAct`` with 32 groups, ``MaxPool2dSame``;
``vision_transformer.py``: ``Block`` / ``Attention`` / ``Mlp`` with LayerNorm eps 1e-6 and exact GELU).  Parity of everything the
reference itself defines is pinned by tests/golden/make_encoder_golden.py, which runs the reference's own modules; the timm-derived
layers cannot be pinned against timm in this image ("parity unpinned" for them).
"""
from __future__ import annotations

import math
from typing import List

import torch
import torch.nn as nn
import torch.nn.functional as F

Tensor = torch.Tensor


# ----------------------------------------------------------------------------------------------------------------------
# timm 0.5.4 layers (restated): weight-standardised convolution with TF "SAME" padding, GroupNorm + ReLU, SAME max-pool
# ----------------------------------------------------------------------------------------------------------------------
def _same_pad(x: Tensor, k: int, s: int, value: float = 0.0) -> Tensor:
    """TF-style SAME padding for a stride-s window of size k: total max((ceil(i/s) - 1) s + k - i, 0), the extra pixel on the
    bottom / right."""
    ih, iw = x.shape[-2:]
    ph = max((math.ceil(ih / s) - 1) * s + k - ih, 0)
    pw = max((math.ceil(iw / s) - 1) * s + k - iw, 0)
    if ph > 0 or pw > 0:
        x = F.pad(x, [pw // 2, pw - pw // 2, ph // 2, ph - ph // 2], value=value)
    return x


class StdConv2dSame(nn.Conv2d):
    """Conv2d whose weight is standardised per output channel (zero mean, unit biased variance over in x kh x kw, ``eps`` inside the
    square root) on every forward; SAME padding: static (k - 1) / 2 at stride 1, dynamic (input-size dependent) otherwise."""

    def __init__(self, in_ch: int, out_ch: int, kernel_size: int, stride: int = 1, eps: float = 1e-6):
        static = stride == 1
        super().__init__(in_ch, out_ch, kernel_size, stride=stride, padding=(kernel_size - 1) // 2 if static else 0, bias=False)
        self.dynamic_pad = not static
        self.eps = eps

    def forward(self, x: Tensor) -> Tensor:
        if self.dynamic_pad:
            x = _same_pad(x, self.kernel_size[0], self.stride[0])
        w = self.weight.reshape(self.out_channels, -1)
        var, mean = torch.var_mean(w, dim=1, unbiased=False, keepdim=True)
        w = ((w - mean) * torch.rsqrt(var + self.eps)).reshape_as(self.weight)
        return F.conv2d(x, w, None, self.stride, self.padding)


class GroupNormAct(nn.GroupNorm):
    def __init__(self, channels: int, apply_act: bool = True):
        super().__init__(32, channels, eps=1e-5)
        self.apply_act = apply_act

    def forward(self, x: Tensor) -> Tensor:
        x = F.group_norm(x, self.num_groups, self.weight, self.bias, self.eps)
        return F.relu(x) if self.apply_act else x


class MaxPool2dSame(nn.Module):
    def forward(self, x: Tensor) -> Tensor:
        return F.max_pool2d(_same_pad(x, 3, 2, value=-float("inf")), 3, 2)


class _Downsample(nn.Module):
    def __init__(self, in_ch: int, out_ch: int, stride: int):
        super().__init__()
        self.conv = StdConv2dSame(in_ch, out_ch, 1, stride=stride, eps=1e-8)
        self.norm = GroupNormAct(out_ch, apply_act=False)

    def forward(self, x: Tensor) -> Tensor:
        return self.norm(self.conv(x))


class Bottleneck(nn.Module):
    """timm resnetv2 ``Bottleneck`` (the non-pre-activation block used for ViT hybrids): 1x1 -> 3x3 (stride) -> 1x1, GroupNorm after
    every convolution, ReLU after the first two and after the residual sum."""

    def __init__(self, in_ch: int, out_ch: int, stride: int, project: bool):
        super().__init__()
        mid = out_ch // 4
        self.downsample = _Downsample(in_ch, out_ch, stride) if project else None
        self.conv1 = StdConv2dSame(in_ch, mid, 1, eps=1e-8)
        self.norm1 = GroupNormAct(mid)
        self.conv2 = StdConv2dSame(mid, mid, 3, stride=stride, eps=1e-8)
        self.norm2 = GroupNormAct(mid)
        self.conv3 = StdConv2dSame(mid, out_ch, 1, eps=1e-8)
        self.norm3 = GroupNormAct(out_ch, apply_act=False)

    def forward(self, x: Tensor) -> Tensor:
        shortcut = x if self.downsample is None else self.downsample(x)
        x = self.norm1(self.conv1(x))
        x = self.norm2(self.conv2(x))
        x = self.norm3(self.conv3(x))
        return F.relu(x + shortcut)


class _Stage(nn.Module):
    def __init__(self, in_ch: int, out_ch: int, stride: int, depth: int):
        super().__init__()
        self.blocks = nn.Sequential(*[Bottleneck(in_ch if i == 0 else out_ch, out_ch, stride if i == 0 else 1, project=(i == 0))
                                      for i in range(depth)])

    def forward(self, x: Tensor) -> Tensor:
        return self.blocks(x)


class ResNetV2Trunk(nn.Module):
    """``timm.models.vision_transformer_hybrid._resnetv2((3, 4, 9))``: stem (7x7 stride 2, GroupNorm+ReLU, SAME max-pool) and three
    stages of 256 / 512 / 1024 channels at strides 4 / 8 / 16.  The reference replaces the stem convolution by a fresh
    ``StdConv2dSame(3, 64, 7, stride 2)`` with the class default eps 1e-6 (models.py:93)."""

    def __init__(self):
        super().__init__()
        self.stem = nn.Sequential()
        self.stem.add_module("conv", StdConv2dSame(3, 64, 7, stride=2, eps=1e-6))
        self.stem.add_module("norm", GroupNormAct(64))
        self.stem.add_module("pool", MaxPool2dSame())
        self.stages = nn.Sequential(_Stage(64, 256, 1, 3), _Stage(256, 512, 2, 4), _Stage(512, 1024, 2, 9))

    def forward(self, x: Tensor) -> List[Tensor]:
        x = self.stem(x)
        feats = []
        for stage in self.stages:
            x = stage(x)
            feats.append(x)
        return feats


class HybridEmbed(nn.Module):
    def __init__(self, embed_dim: int = 768):
        super().__init__()
        self.backbone = ResNetV2Trunk()
        self.proj = nn.Conv2d(1024, embed_dim, kernel_size=1, stride=1)


# ----------------------------------------------------------------------------------------------------------------------
# timm 0.5.4 transformer block (restated)
# ----------------------------------------------------------------------------------------------------------------------
class Attention(nn.Module):
    def __init__(self, dim: int, heads: int):
        super().__init__()
        self.heads = heads
        self.qkv = nn.Linear(dim, dim * 3, bias=True)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x: Tensor) -> Tensor:
        B, N, C = x.shape
        q, k, v = self.qkv(x).reshape(B, N, 3, self.heads, C // self.heads).permute(2, 0, 3, 1, 4).unbind(0)
        x = F.scaled_dot_product_attention(q, k, v)            # softmax(q k^T / sqrt(head_dim)) v
        return self.proj(x.transpose(1, 2).reshape(B, N, C))


class Mlp(nn.Module):
    def __init__(self, dim: int, hidden: int):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x: Tensor) -> Tensor:
        return self.fc2(F.gelu(self.fc1(x)))


class Block(nn.Module):
    def __init__(self, dim: int, heads: int):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = Attention(dim, heads)
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = Mlp(dim, 4 * dim)

    def forward(self, x: Tensor) -> Tensor:
        x = x + self.attn(self.norm1(x))
        return x + self.mlp(self.norm2(x))


class MultiViewViT(nn.Module):
    """``VisionTransformerMultiView`` (vit_models.py:10-97) with the reference's ``forward_flex`` (midas/vit.py:124-202): parameter
    holder for ``encoder.pretrained.model.*``.  ``head`` (768 -> 1000) and ``pos_embed_second`` exist in the reference's state_dict
    and have no effect on the features."""

    def __init__(self, embed_dim: int = 768, depth: int = 12, heads: int = 12, grid: int = 24):
        super().__init__()
        self.patch_embed = HybridEmbed(embed_dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, grid * grid + 1, embed_dim))
        self.pos_embed_second = nn.Parameter(torch.zeros(1, grid * grid + 1, embed_dim))
        self.blocks = nn.Sequential(*[Block(embed_dim, heads) for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim, eps=1e-6)
        self.pose_embed = nn.Linear(16, embed_dim)
        self.head = nn.Linear(embed_dim, 1000)
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        nn.init.trunc_normal_(self.pos_embed_second, std=0.02)
        nn.init.trunc_normal_(self.cls_token, std=0.02)

    def resized_pos_embed(self, gh: int, gw: int) -> Tensor:
        """Class-token entry kept, grid entries bilinearly resized to gh x gw (midas/vit.py:107-121)."""
        tok, grid = self.pos_embed[:, :1], self.pos_embed[0, 1:]
        g = int(math.sqrt(grid.shape[0]))
        grid = F.interpolate(grid.reshape(1, g, g, -1).permute(0, 3, 1, 2), size=(gh, gw), mode="bilinear")
        return torch.cat([tok, grid.permute(0, 2, 3, 1).reshape(1, gh * gw, -1)], dim=1)


class ProjectReadout(nn.Module):
    """Concatenates the class token to every patch token and projects back to the token width (midas/vit.py:31-42)."""

    def __init__(self, dim: int):
        super().__init__()
        self.project = nn.Sequential(nn.Linear(2 * dim, dim), nn.GELU())

    def forward(self, x: Tensor) -> Tensor:
        readout = x[:, :1].expand(-1, x.shape[1] - 1, -1)
        return self.project(torch.cat((x[:, 1:], readout), -1))


class _Pretrained(nn.Module):
    """``encoder.pretrained``: the transformer plus the re-assembly heads of taps 3 and 4 (midas/vit.py:482-513); taps 1 and 2 are the
    ResNet stages themselves (identity post-processing, midas/vit.py:474-480).  Sequential indices follow the reference so that the
    checkpoint keys match: [0] readout, [1] transpose, [2] unflatten, [3] 1x1 conv, ([4] 3x3 stride-2 conv)."""

    def __init__(self, dim: int = 768):
        super().__init__()
        self.model = MultiViewViT(dim)
        self.act_postprocess3 = nn.Sequential(ProjectReadout(dim), nn.Identity(), nn.Identity(), nn.Conv2d(dim, 768, 1))
        self.act_postprocess4 = nn.Sequential(ProjectReadout(dim), nn.Identity(), nn.Identity(), nn.Conv2d(dim, 768, 1),
                                              nn.Conv2d(768, 768, 3, stride=2, padding=1))


# ----------------------------------------------------------------------------------------------------------------------
# RefineNet fusion (midas/blocks.py:231-341) and the DPT wrapper
# ----------------------------------------------------------------------------------------------------------------------
class ResidualConvUnit(nn.Module):
    def __init__(self, ch: int):
        super().__init__()
        self.conv1 = nn.Conv2d(ch, ch, 3, padding=1)
        self.conv2 = nn.Conv2d(ch, ch, 3, padding=1)

    def forward(self, x: Tensor) -> Tensor:
        return self.conv2(F.relu(self.conv1(F.relu(x)))) + x


class FeatureFusionBlock(nn.Module):
    def __init__(self, ch: int):
        super().__init__()
        self.out_conv = nn.Conv2d(ch, ch, 1)
        self.resConfUnit1 = ResidualConvUnit(ch)
        self.resConfUnit2 = ResidualConvUnit(ch)

    def forward(self, x: Tensor, skip: Tensor = None) -> Tensor:
        if skip is not None:
            x = x + self.resConfUnit1(skip)
        x = self.resConfUnit2(x)
        x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
        return self.out_conv(x)


class _Scratch(nn.Module):
    def __init__(self, ch: int = 256):
        super().__init__()
        for i, c in enumerate((256, 512, 768, 768), start=1):
            setattr(self, f"layer{i}_rn", nn.Conv2d(c, ch, 3, padding=1, bias=False))
        for i in range(1, 5):
            setattr(self, f"refinenet{i}", FeatureFusionBlock(ch))
        # the monocular-depth head of DPTDepthModel (midas/dpt_depth.py:98-106): in the checkpoint, never evaluated by get_z
        self.output_conv = nn.Sequential(nn.Conv2d(ch, ch // 2, 3, padding=1), nn.Identity(), nn.Conv2d(ch // 2, 32, 3, padding=1),
                                         nn.Identity(), nn.Conv2d(32, 1, 1), nn.Identity(), nn.Identity())


class _VitBlocksTrain(torch.autograd.Function):
    """The 12 blocks as one autograd node over (tok, the 144 block parameters): car_vit_blocks_train forward, car_vit_blocks_backward
    backward (include/car_encoder_train.h).  Once differentiable: a double backward raises.

    The parameters are packed afresh on every forward (car_vit_pack_train: the forward's layout and the transposed matrices of
    dX = dY W): the packed cache of the inference route keys on the tensors' _version, which torch's fused optimizers do not advance, so
    between two training steps it would hand back the old weights.  The parameter gradients come back as views of ONE flat buffer
    (car_vit_grad_offset's layout), as training.render_train's do; autograd's accumulation into .grad is the usual one, so two backwards
    without zero_grad add up.  The LayerNorm gradients and the gradient of tok are bit-reproducible; the matrices' and their biases' go
    through car_linear_wgrad's fp32 atomics and are reproducible to rounding."""

    @staticmethod
    def forward(ctx, enc, BV, T, tok, *params):
        import ctypes
        from . import _lib
        lib, dev = _lib.api(), tok.device
        b, S, dim = tok.shape
        depth, taps = len(params) // 12, enc.VIT_TAPS
        f32 = dict(device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            packed = torch.empty(_lib.user_call(lib.car_vit_packed_train_floats, dim, depth), **f32)
            src = [p.detach().contiguous() for p in params]
            _lib.user_call(lib.car_vit_pack_train, (ctypes.c_void_p * len(src))(*[t.data_ptr() for t in src]), len(src), dim, depth, _lib.ptr(packed),
                           _lib.stream())
            saved = torch.empty(_lib.user_call(lib.car_vit_saved_bytes, b, S, dim, depth) // 4, **f32)
            work = enc._vit_workspace(lib, b, S, dim, dev)
            x = tok.detach().clone(memory_format=torch.contiguous_format)     # the stage runs in place
            outs = [torch.empty(BV, T, dim, **f32) for _ in taps]
            _lib.user_call(lib.car_vit_blocks_train, _lib.ptr(x), b, S, dim, _lib.ptr(packed), depth, (ctypes.c_int * len(taps))(*taps), len(taps),
                           (ctypes.c_void_p * len(outs))(*[t.data_ptr() for t in outs]), _lib.ptr(saved), saved.numel() * 4, _lib.ptr(work),
                           work.numel() * 4, _lib.stream())
        ctx.packed, ctx.saved, ctx.shape, ctx.taps, ctx.params = packed, saved, (b, S, dim, depth), taps, params
        # the record lives in plain buffers autograd does not track: an in-place parameter update between forward and backward is
        # checked by hand, as training.render_train does
        ctx.param_versions = [p._version for p in params]
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *dtaps):
        import ctypes
        from . import _lib
        stale = [i for i, (p, v) in enumerate(zip(ctx.params, ctx.param_versions)) if p._version != v]
        if stale:
            raise RuntimeError(f"vit_route = 'device_train': block parameters were modified in place between forward and backward (blocks "
                               f"{sorted({i // 12 for i in stale})[:3]} ...): the saved activations no longer belong to them")
        lib, dev = _lib.api(), ctx.saved.device
        b, S, dim, depth = ctx.shape
        f32 = dict(device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            off = [lib.car_vit_grad_offset(dim, i) for i in range(13)]
            flat = torch.zeros(depth * off[12], **f32)                         # the entry adds the matrices' gradients: zeroed here
            dtok = torch.zeros(b, S, dim, **f32)                               # the stage's own output is not an output of this node
            work = torch.empty(_lib.user_call(lib.car_vit_backward_workspace_bytes, b, S, dim) // 4, **f32)
            d = [None if t is None else t.to(torch.float32).contiguous() for t in dtaps]
            _lib.user_call(lib.car_vit_blocks_backward, _lib.ptr(dtok), b, S, dim, _lib.ptr(ctx.packed), depth, (ctypes.c_int * len(d))(*ctx.taps), len(d),
                           (ctypes.c_void_p * len(d))(*[None if t is None else t.data_ptr() for t in d]), _lib.ptr(ctx.saved), ctx.saved.numel() * 4,
                           _lib.ptr(flat), 0, _lib.ptr(work), work.numel() * 4, _lib.stream())
        grads = [flat[(i // 12) * off[12] + off[i % 12]:][:p.numel()].view_as(p) if ctx.needs_input_grad[4 + i] else None
                 for i, p in enumerate(ctx.params)]
        ctx.packed = ctx.saved = None
        return (None, None, None, dtok if ctx.needs_input_grad[3] else None, *grads)


class MultiViewDPTEncoder(nn.Module):
    """Drop-in for the reference's ``self.encoder`` when ``model == "midas_vit"`` (models.py:82-94): same parameter names, same
    ``forward(rgb, rel_pose16, nviews) -> [path_2, path_1]``."""

    TOKENS_PER_VIEW = 257          # `os = 257` in the reference's forward_flex (midas/vit.py:183): 16 x 16 patches + class token
    VIT_TAPS = (8, 11)             # the blocks whose outputs are re-assembled (midas/vit.py:65-69)
    VIT_ROUTES = ("torch", "device")
    VIT_BLOCK_ROUTES = ("torch", "device", "device_train")   # vit_route's own values: the blocks also have a recorded forward and a backward
    TRUNK_DEPTHS = (3, 4, 9)       # the stages of ResNetV2Trunk, as car_trunk_pack takes them

    def __init__(self):
        super().__init__()
        self.pretrained = _Pretrained()
        self.scratch = _Scratch()
        # where the transformer blocks run: "torch" (the default: the modules above) or the opt-in "device" (car_vit_blocks on the packed
        # parameters: inference only, float32 CUDA tensors only; it refuses anything else instead of falling back) or the opt-in
        # "device_train" (under no_grad the "device" route, call for call; where autograd records, car_vit_blocks_train with
        # car_vit_blocks_backward as its backward: _VitBlocksTrain below)
        self.vit_route = "torch"
        self._vit_packed = None    # engine._Cached of the packed blocks (source: their 144 parameter tensors), made on first use
        self._vit_work = {}        # (b, S, device) -> the stage's workspace on the device
        # where the ResNetV2 trunk and the token assembly run: "torch" (the default) or the opt-in "device" (car_trunk_forward and
        # car_vit_tokens on the packed parameters; the same conditions and the same refusals as vit_route, and independent of it)
        self.trunk_route = "torch"
        self._trunk_packed = None  # engine._Cached of the packed trunk (source: its parameter tensors in state_dict order)
        self._tokens_packed = None # engine._Cached of the packed token parameters (projection, class token, position and pose embeddings)
        self._trunk_work = {}      # (BV, H, W, device) -> (the trunk's workspace, the token assembly's workspace)
        # where the read-out, the re-assembly and the fusion run: "torch" (the default) or the opt-in "device" (car_decoder_forward on the
        # packed parameters; the same conditions and the same refusals as the other two switches, and independent of them)
        self.decoder_route = "torch"
        self._decoder_packed = None  # engine._Cached of the packed decoder (source: the 50 parameter tensors it evaluates)
        self._decoder_work = {}      # (BV, gh, gw, device) -> the decoder's workspace

    @property
    def vit_route(self) -> str:
        return self._vit_route

    @vit_route.setter
    def vit_route(self, value: str) -> None:
        if value not in self.VIT_BLOCK_ROUTES:
            raise ValueError(f"vit_route must be 'torch', 'device' or 'device_train' (got {value!r})")
        self._vit_route = value

    @property
    def trunk_route(self) -> str:
        return self._trunk_route

    @trunk_route.setter
    def trunk_route(self, value: str) -> None:
        if value not in self.VIT_ROUTES:
            raise ValueError(f"trunk_route must be 'torch' or 'device' (got {value!r})")
        self._trunk_route = value

    @property
    def decoder_route(self) -> str:
        return self._decoder_route

    @decoder_route.setter
    def decoder_route(self, value: str) -> None:
        if value not in self.VIT_ROUTES:
            raise ValueError(f"decoder_route must be 'torch' or 'device' (got {value!r})")
        self._decoder_route = value

    def drop_device_caches(self) -> None:
        """Forgets the packed blocks, the packed trunk and token parameters, the packed decoder and the workspaces: the next device-route forward packs the
        parameters as they are then.  The cache's key sees an in-place update through the tensors' _version, which torch's fused optimizers
        do not advance (CrossAttentionRenderer.train calls this on leaving train() mode, as it parks the engine's caches)."""
        for cached in (self._vit_packed, self._trunk_packed, self._tokens_packed, self._decoder_packed):
            if cached is not None:
                cached.drop()
        self._vit_work = {}
        self._trunk_work = {}
        self._decoder_work = {}

    def _trunk_parameters(self) -> List[Tensor]:
        """The trunk's parameters in car_trunk_pack's order: state_dict order of ResNetV2Trunk."""
        return [p for _, p in self.pretrained.model.patch_embed.backbone.named_parameters()]

    def _token_parameters(self) -> List[Tensor]:
        """car_vit_tokens_pack's six arrays: the projection, the class token, the position embedding, the pose embedding."""
        vit = self.pretrained.model
        return [vit.patch_embed.proj.weight, vit.patch_embed.proj.bias, vit.cls_token, vit.pos_embed, vit.pose_embed.weight, vit.pose_embed.bias]

    def _front_on_device(self, x: Tensor, rel_pose16: Tensor, gh: int, gw: int):
        """The trunk and the token assembly through car_trunk_forward and car_vit_tokens: x [BV, 3, H, W] ->
        (layer_1 [BV, 256, H/4, W/4], layer_2 [BV, 512, H/8, W/8] — NCHW views of the channel-last buffers — and tok [BV, 1 + gh gw, 768])."""
        import ctypes
        from . import _lib
        from .engine import _Cached
        trunk, toks = self._trunk_parameters(), self._token_parameters()
        params = trunk + toks
        if not x.is_cuda or not rel_pose16.is_cuda or not all(p.is_cuda for p in params):
            raise ValueError("trunk_route = 'device' needs the images and the encoder on a CUDA device; CPU tensors run on trunk_route = 'torch'")
        if x.dtype != torch.float32 or rel_pose16.dtype != torch.float32 or any(p.dtype != torch.float32 for p in params):
            raise ValueError(f"trunk_route = 'device' computes in float32 (got {x.dtype}); other dtypes run on trunk_route = 'torch'")
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise ValueError("trunk_route = 'device' is inference only (its kernels have no backward): call it under torch.no_grad(), or "
                             "keep trunk_route = 'torch' for a forward that autograd records")
        lib, dev = _lib.api(), x.device
        BV, _, H, W = x.shape
        depths = (ctypes.c_int * 3)(*self.TRUNK_DEPTHS)
        grid = int(math.sqrt(toks[3].shape[1] - 1))
        if self._trunk_packed is None:
            self._trunk_packed, self._tokens_packed = _Cached(), _Cached()

        def build_trunk():
            packed = torch.empty(_lib.user_call(lib.car_trunk_packed_floats, depths), device=dev, dtype=torch.float32)
            src = [p.detach().contiguous() for p in trunk]
            _lib.user_call(lib.car_trunk_pack, (ctypes.c_void_p * len(src))(*[t.data_ptr() for t in src]), len(src), depths, _lib.ptr(packed), _lib.stream())
            return packed

        def build_tokens():
            packed = torch.empty(_lib.user_call(lib.car_vit_tokens_packed_floats, gh, gw), device=dev, dtype=torch.float32)
            pw, pb, cls, pos, sw, sb = [p.detach().contiguous() for p in toks]
            _lib.user_call(lib.car_vit_tokens_pack, _lib.ptr(pw), _lib.ptr(pb), _lib.ptr(cls), _lib.ptr(pos), grid, _lib.ptr(sw), _lib.ptr(sb), gh, gw,
                           _lib.ptr(packed), _lib.stream())
            return packed
        with torch.cuda.device(dev):
            packed = self._trunk_packed.get(trunk, (str(dev), self.TRUNK_DEPTHS), build_trunk)
            tpacked = self._tokens_packed.get(toks, (str(dev), gh, gw), build_tokens)
            key = (BV, H, W, str(dev))
            if key not in self._trunk_work:
                self._trunk_work = {key: (torch.empty(_lib.user_call(lib.car_trunk_workspace_bytes, BV, H, W, depths) // 4, device=dev, dtype=torch.float32),
                                          torch.empty(_lib.user_call(lib.car_vit_tokens_workspace_bytes, BV, gh, gw) // 4, device=dev, dtype=torch.float32))}
            work, twork = self._trunk_work[key]
            up = lambda v, k: -(-v // k)
            h4, w4, h8, w8, h16, w16 = up(H, 4), up(W, 4), up(H, 8), up(W, 8), up(H, 16), up(W, 16)
            if (h16, w16) != (gh, gw):
                raise ValueError(f"trunk_route = 'device': a {H}x{W} image gives {h16}x{w16} trunk features, not the {gh}x{gw} token grid")
            layer_1 = torch.empty(BV, h4, w4, 256, device=dev, dtype=torch.float32)
            layer_2 = torch.empty(BV, h8, w8, 512, device=dev, dtype=torch.float32)
            feat = torch.empty(BV, h16 * w16, 1024, device=dev, dtype=torch.float32)
            tok = torch.empty(BV, 1 + gh * gw, 768, device=dev, dtype=torch.float32)
            xc, pose = x.contiguous(), rel_pose16.contiguous()
            _lib.user_call(lib.car_trunk_forward, _lib.ptr(xc), BV, H, W, _lib.ptr(packed), depths, _lib.ptr(layer_1), _lib.ptr(layer_2), _lib.ptr(feat),
                           _lib.ptr(work), work.numel() * 4, _lib.stream())
            _lib.user_call(lib.car_vit_tokens, _lib.ptr(feat), BV, gh, gw, _lib.ptr(pose), _lib.ptr(tpacked), _lib.ptr(tok), _lib.ptr(twork),
                           twork.numel() * 4, _lib.stream())
        return layer_1.permute(0, 3, 1, 2), layer_2.permute(0, 3, 1, 2), tok      # NCHW views: torch's convolutions take channels_last

    def _vit_parameters(self) -> List[Tensor]:
        """The blocks' parameters in car_vit_pack's order (12 per block)."""
        names = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
                 "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")
        return [blk.get_parameter(n) for blk in self.pretrained.model.blocks for n in names]

    def _refuse_off_device(self, tok: Tensor, params: List[Tensor]) -> None:
        """What both device routes of the blocks refuse instead of falling back: CPU tensors, other dtypes."""
        if not tok.is_cuda or not all(p.is_cuda for p in params):
            raise ValueError(f"vit_route = {self.vit_route!r} needs the images and the encoder on a CUDA device; CPU tensors run on vit_route = 'torch'")
        if tok.dtype != torch.float32 or any(p.dtype != torch.float32 for p in params):
            raise ValueError(f"vit_route = {self.vit_route!r} computes in float32 (got {tok.dtype}); other dtypes run on vit_route = 'torch'")

    def _vit_workspace(self, lib, b: int, S: int, dim: int, dev) -> Tensor:
        key = (b, S, str(dev))
        if key not in self._vit_work:
            self._vit_work = {key: torch.empty(lib.car_vit_workspace_bytes(b, S, dim) // 4, device=dev, dtype=torch.float32)}
        return self._vit_work[key]

    def _blocks_recorded_on_device(self, tok: Tensor, BV: int, T: int) -> dict:
        """The transformer stage where autograd records (vit_route = "device_train"): car_vit_blocks_train, with car_vit_blocks_backward
        as its backward.  tok [b, V T, dim] -> {tap: [BV, T, dim]}, each carrying the gradient back to tok and to the 144 block parameters."""
        params = self._vit_parameters()
        self._refuse_off_device(tok, params)
        outs = _VitBlocksTrain.apply(self, BV, T, tok, *params)
        return dict(zip(self.VIT_TAPS, outs))

    def _blocks_on_device(self, tok: Tensor, x: Tensor, BV: int, T: int) -> dict:
        """The transformer stage through car_vit_blocks: tok [b, V T, dim] (contiguous, overwritten) -> {tap: [BV, T, dim]}."""
        return self._blocks_inference(tok, x, BV, T, False)

    def _blocks_inference(self, tok: Tensor, x: Tensor, BV: int, T: int, recorded_elsewhere: bool) -> dict:
        """_blocks_on_device's body.  recorded_elsewhere (vit_route = "device_train" only): grad mode may be on, but neither tok nor a block
        parameter asks for a gradient, so nothing would flow through the blocks — the inference call is the whole of it."""
        import ctypes
        from . import _lib
        from .engine import _Cached
        params = self._vit_parameters()
        self._refuse_off_device(tok, params)
        if not recorded_elsewhere and torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise ValueError("vit_route = 'device' is inference only (its kernels have no backward): call it under torch.no_grad(), or "
                             "keep vit_route = 'torch' for a forward that autograd records")
        lib, dev = _lib.api(), tok.device
        b, S, dim = tok.shape
        depth = len(params) // 12
        if self._vit_packed is None:
            self._vit_packed = _Cached()

        def build():
            packed = torch.empty(_lib.user_call(lib.car_vit_packed_floats, dim, depth), device=dev, dtype=torch.float32)
            src = [p.detach().contiguous() for p in params]
            _lib.user_call(lib.car_vit_pack, (ctypes.c_void_p * len(src))(*[t.data_ptr() for t in src]), len(src), dim, depth, _lib.ptr(packed),
                           _lib.stream())
            return packed
        with torch.cuda.device(dev):
            packed = self._vit_packed.get(params, (str(dev), dim, depth), build)
            work = self._vit_workspace(lib, b, S, dim, dev)
            outs = [torch.empty(BV, T, dim, device=dev, dtype=torch.float32) for _ in self.VIT_TAPS]
            _lib.user_call(lib.car_vit_blocks, _lib.ptr(tok), b, S, dim, _lib.ptr(packed), depth, (ctypes.c_int * len(outs))(*self.VIT_TAPS),
                           len(outs), (ctypes.c_void_p * len(outs))(*[t.data_ptr() for t in outs]), _lib.ptr(work), work.numel() * 4,
                           _lib.stream())
        return dict(zip(self.VIT_TAPS, outs))

    def _decoder_parameters(self) -> List[Tensor]:
        """The 50 parameters the decoder evaluates, in car_decoder_pack's order: state_dict order without refinenet4.resConfUnit1 and
        scratch.output_conv, which get_z never evaluates."""
        pre, s = self.pretrained, self.scratch
        mods = [pre.act_postprocess3[0].project[0], pre.act_postprocess3[3], pre.act_postprocess4[0].project[0], pre.act_postprocess4[3], pre.act_postprocess4[4]]
        params = [p for m in mods for p in (m.weight, m.bias)] + [getattr(s, f"layer{i}_rn").weight for i in range(1, 5)]
        for i in range(1, 5):
            r = getattr(s, f"refinenet{i}")
            convs = [r.out_conv] + ([r.resConfUnit1.conv1, r.resConfUnit1.conv2] if i < 4 else []) + [r.resConfUnit2.conv1, r.resConfUnit2.conv2]
            params += [p for m in convs for p in (m.weight, m.bias)]
        return params

    def _back_on_device(self, tap3: Tensor, tap4: Tensor, layer_1: Tensor, layer_2: Tensor, x: Tensor, gh: int, gw: int) -> List[Tensor]:
        """The read-out, the re-assembly and the fusion through car_decoder_forward: the two tapped states [BV, 1 + gh gw, 768] and the trunk's
        first two stage ends (NCHW) -> [path_2 [BV, 256, 4gh, 4gw], path_1 [BV, 256, 8gh, 8gw]], NCHW views of the channel-last buffers."""
        import ctypes
        from . import _lib
        from .engine import _Cached
        params = self._decoder_parameters()
        acts = (tap3, tap4, layer_1, layer_2)
        if not all(t.is_cuda for t in acts) or not all(p.is_cuda for p in params):
            raise ValueError("decoder_route = 'device' needs the images and the encoder on a CUDA device; CPU tensors run on decoder_route = 'torch'")
        if any(t.dtype != torch.float32 for t in acts) or any(p.dtype != torch.float32 for p in params):
            raise ValueError(f"decoder_route = 'device' computes in float32 (got {tap3.dtype}); other dtypes run on decoder_route = 'torch'")
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise ValueError("decoder_route = 'device' is inference only (its kernels have no backward): call it under torch.no_grad(), or "
                             "keep decoder_route = 'torch' for a forward that autograd records")
        lib, dev = _lib.api(), tap3.device
        BV = tap3.shape[0]
        if self._decoder_packed is None:
            self._decoder_packed = _Cached()

        def build():
            packed = torch.empty(_lib.user_call(lib.car_decoder_packed_floats), device=dev, dtype=torch.float32)
            src = [p.detach().contiguous() for p in params]
            _lib.user_call(lib.car_decoder_pack, (ctypes.c_void_p * len(src))(*[t.data_ptr() for t in src]), len(src), _lib.ptr(packed), _lib.stream())
            return packed
        with torch.cuda.device(dev):
            packed = self._decoder_packed.get(params, (str(dev),), build)
            key = (BV, gh, gw, str(dev))
            if key not in self._decoder_work:
                self._decoder_work = {key: torch.empty(_lib.user_call(lib.car_decoder_workspace_bytes, BV, gh, gw) // 4, device=dev, dtype=torch.float32)}
            work = self._decoder_work[key]
            if tuple(layer_1.shape[-2:]) != (4 * gh, 4 * gw) or tuple(layer_2.shape[-2:]) != (2 * gh, 2 * gw):
                raise ValueError(f"decoder_route = 'device': stage ends of {tuple(layer_1.shape[-2:])} and {tuple(layer_2.shape[-2:])} are not 4 and 2 times "
                                 f"the {gh}x{gw} token grid")
            l1, l2 = layer_1.permute(0, 2, 3, 1).contiguous(), layer_2.permute(0, 2, 3, 1).contiguous()     # no copy behind trunk_route = 'device'
            t3, t4 = tap3.contiguous(), tap4.contiguous()
            path_2 = torch.empty(BV, 4 * gh, 4 * gw, 256, device=dev, dtype=torch.float32)
            path_1 = torch.empty(BV, 8 * gh, 8 * gw, 256, device=dev, dtype=torch.float32)
            _lib.user_call(lib.car_decoder_forward, _lib.ptr(t3), _lib.ptr(t4), _lib.ptr(l1), _lib.ptr(l2), BV, gh, gw, _lib.ptr(packed), _lib.ptr(path_2),
                           _lib.ptr(path_1), _lib.ptr(work), work.numel() * 4, _lib.stream())
        return [path_2.permute(0, 3, 1, 2), path_1.permute(0, 3, 1, 2)]          # NCHW views: the engine takes channels_last without a copy

    def forward(self, x: Tensor, rel_pose16: Tensor, nviews: int) -> List[Tensor]:
        vit = self.pretrained.model
        BV, _, H, W = x.shape
        gh, gw = H // 16, W // 16
        if gh * gw + 1 != self.TOKENS_PER_VIEW:
            raise ValueError(f"the multi-view encoder splits the token sequence at {self.TOKENS_PER_VIEW} tokens per view "
                             f"(midas/vit.py:183, 199): only 256x256 inputs work, got {H}x{W}")
        if BV % nviews:
            raise ValueError("batch of views is not a multiple of nviews")
        if self.trunk_route == "device":
            layer_1, layer_2, tok = self._front_on_device(x, rel_pose16, gh, gw)   # a missing kernel or a refused input raises: no fallback
        else:
            layer_1, layer_2, feat = vit.patch_embed.backbone(x)               # 256 @ H/4, 512 @ H/8, 1024 @ H/16
            tok = vit.patch_embed.proj(feat).flatten(2).transpose(1, 2)        # (BV, gh*gw, 768)
            tok = torch.cat((vit.cls_token.expand(BV, -1, -1), tok), dim=1)
            tok = tok + vit.resized_pos_embed(gh, gw) + vit.pose_embed(rel_pose16)[:, None, :]
        T = tok.shape[1]
        tok = tok.view(BV // nviews, nviews * T, -1)                           # all views of a scene in one sequence
        records = self.vit_route == "device_train" and torch.is_grad_enabled() and (tok.requires_grad or any(p.requires_grad for p in self._vit_parameters()))
        if records:
            taps = self._blocks_recorded_on_device(tok, BV, T)                 # a missing kernel or a refused input raises: no fallback
        elif self.vit_route == "device_train":
            taps = self._blocks_inference(tok.contiguous(), x, BV, T, True)    # nothing to record: the "device" route's own call
        elif self.vit_route == "device":
            taps = self._blocks_on_device(tok.contiguous(), x, BV, T)          # a missing kernel or a refused input raises: no fallback
        else:
            taps = {}
            for i, blk in enumerate(vit.blocks):
                tok = blk(tok)
                if i in self.VIT_TAPS:
                    taps[i] = tok.reshape(BV, T, -1)                           # back to one row per view (midas/vit.py:65-69)
        if self.decoder_route == "device":
            return self._back_on_device(taps[8], taps[11], layer_1, layer_2, x, gh, gw)   # a missing kernel or a refused input raises: no fallback

        def reassemble(t: Tensor, post: nn.Sequential) -> Tensor:
            t = post[0](t).transpose(1, 2).unflatten(2, (gh, gw))
            for layer in post[3:]:
                t = layer(t)
            return t
        layer_3 = reassemble(taps[8], self.pretrained.act_postprocess3)        # 768 @ H/16
        layer_4 = reassemble(taps[11], self.pretrained.act_postprocess4)       # 768 @ H/32
        s = self.scratch
        path_4 = s.refinenet4(s.layer4_rn(layer_4))
        path_3 = s.refinenet3(path_4, s.layer3_rn(layer_3))
        path_2 = s.refinenet2(path_3, s.layer2_rn(layer_2))
        path_1 = s.refinenet1(path_2, s.layer1_rn(layer_1))
        return [path_2, path_1]
