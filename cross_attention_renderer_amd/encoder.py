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

import ctypes
import itertools
import math
from typing import Callable, Iterable, List, Optional, Sequence

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


# ----------------------------------------------------------------------------------------------------------------------
# The host plumbing of get_z's device stages, stated once: the refusals, the pack, the route switches (the cached slots and the
# workspaces are methods of MultiViewDPTEncoder below).  A new device stage uses these and states none of it again
# ----------------------------------------------------------------------------------------------------------------------
def refuse_off_device(switch: str, value: str, acts: Sequence[Tensor], params: Sequence[Tensor], recorded: Optional[Iterable[Tensor]],
                      model: str = "the encoder", call: str = "call it", inference: Optional[str] = None) -> None:
    """What a device stage behind `switch` (now `value`) refuses instead of falling back, in this order: activations or parameters off a
    CUDA device; a dtype other than float32 (the first activation's is the one reported); and a forward that autograd records — grad mode
    on and any tensor of `recorded` asking for a gradient (None: the stage has a backward, or the caller saw to it).  `inference` names the
    inference-only value where `value` may be another one (vit_route's 'device_train'); `model` and `call` are the texts' two nouns."""
    if not all(t.is_cuda for t in (*acts, *params)):
        raise ValueError(f"{switch} = {value!r} needs the images and {model} on a CUDA device; CPU tensors run on {switch} = 'torch'")
    if any(t.dtype != torch.float32 for t in (*acts, *params)):
        raise ValueError(f"{switch} = {value!r} computes in float32 (got {acts[0].dtype}); other dtypes run on {switch} = 'torch'")
    if recorded is not None and torch.is_grad_enabled() and any(t.requires_grad for t in recorded):
        raise ValueError(f"{switch} = {inference or value!r} is inference only (its kernels have no backward): {call} under torch.no_grad(), or "
                         f"keep {switch} = 'torch' for a forward that autograd records")


def pack_parameters(sources: Sequence[Tensor], dev, floats: int, issue: Callable) -> Tensor:
    """`sources` packed into one new buffer of `floats` floats on `dev`: issue(table, src, packed) calls the stage's pack entry, given the
    sources' detached, contiguous forms `src` and the c_void_p table of their addresses.  Called inside ``torch.cuda.device(dev)``."""
    packed = torch.empty(floats, device=dev, dtype=torch.float32)
    src = [p.detach().contiguous() for p in sources]
    issue((ctypes.c_void_p * len(src))(*[t.data_ptr() for t in src]), src, packed)
    return packed


def _route_switch(name: str, allowed: Sequence[str], text: str) -> property:
    """A route switch: an attribute that takes the values of `allowed` and refuses any other one with `text`."""
    def get(self) -> str:
        return getattr(self, "_" + name)

    def set_(self, value: str) -> None:
        if value not in allowed:
            raise ValueError(f"{name} must be {text} (got {value!r})")
        setattr(self, "_" + name, value)
    return property(get, set_)


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
        from . import _lib
        lib, dev = _lib.api(), tok.device
        b, S, dim = tok.shape
        depth, taps = len(params) // 12, enc.VIT_TAPS
        f32 = dict(device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            packed = pack_parameters(params, dev, _lib.user_call(lib.car_vit_packed_train_floats, dim, depth), lambda table, src, out: _lib.user_call(
                lib.car_vit_pack_train, table, len(src), dim, depth, _lib.ptr(out), _lib.stream()))
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

    # the device stages' caches, by attribute.  Packed parameters: None until first use, then an engine._Cached (_cached below)
    _PACKED_SLOTS = ("_vit_packed",      # the packed blocks (source: their 144 parameter tensors)
                     "_trunk_packed",    # the packed trunk (source: its parameter tensors in state_dict order)
                     "_tokens_packed",   # the packed token parameters (projection, class token, position and pose embeddings)
                     "_decoder_packed")  # the packed decoder (source: the 50 parameter tensors it evaluates)
    # ... and workspaces: a dict of one entry, replaced when the key changes (_workspace below)
    _WORK_SLOTS = ("_vit_work",          # (b, S, device) -> the stage's workspace on the device
                   "_trunk_work",        # (BV, H, W, device) -> the trunk's workspace, the token assembly's workspace
                   "_decoder_work")      # (BV, gh, gw, device) -> the decoder's workspace

    def __init__(self):
        super().__init__()
        self.pretrained = _Pretrained()
        self.scratch = _Scratch()
        # where the transformer blocks run: "torch" (the default: the modules above) or the opt-in "device" (car_vit_blocks on the packed
        # parameters: inference only, float32 CUDA tensors only; it refuses anything else instead of falling back) or the opt-in
        # "device_train" (under no_grad the "device" route, call for call; where autograd records, car_vit_blocks_train with
        # car_vit_blocks_backward as its backward: _VitBlocksTrain above)
        self.vit_route = "torch"
        # where the ResNetV2 trunk and the token assembly run: "torch" (the default) or the opt-in "device" (car_trunk_forward and
        # car_vit_tokens on the packed parameters; the same conditions and the same refusals as vit_route, and independent of it)
        self.trunk_route = "torch"
        # where the read-out, the re-assembly and the fusion run: "torch" (the default) or the opt-in "device" (car_decoder_forward on the
        # packed parameters; the same conditions and the same refusals as the other two switches, and independent of them)
        self.decoder_route = "torch"
        for slot in self._PACKED_SLOTS:
            setattr(self, slot, None)
        for slot in self._WORK_SLOTS:
            setattr(self, slot, {})

    vit_route = _route_switch("vit_route", VIT_BLOCK_ROUTES, "'torch', 'device' or 'device_train'")
    trunk_route = _route_switch("trunk_route", VIT_ROUTES, "'torch' or 'device'")
    decoder_route = _route_switch("decoder_route", VIT_ROUTES, "'torch' or 'device'")

    def drop_device_caches(self) -> None:
        """Forgets the packed blocks, the packed trunk and token parameters, the packed decoder and the workspaces: the next device-route forward packs the
        parameters as they are then.  The cache's key sees an in-place update through the tensors' _version, which torch's fused optimizers
        do not advance (CrossAttentionRenderer.train calls this on leaving train() mode, as it parks the engine's caches)."""
        for slot in self._PACKED_SLOTS:
            if getattr(self, slot) is not None:
                getattr(self, slot).drop()
        for slot in self._WORK_SLOTS:
            setattr(self, slot, {})

    def _cached(self, slot: str, sources: List[Tensor], extra: tuple, build: Callable):
        """The value held in the packed slot `slot` for these sources and plain values (engine._Cached's key rule), built where it is not."""
        from .engine import _Cached
        if getattr(self, slot) is None:
            setattr(self, slot, _Cached())
        return getattr(self, slot).get(sources, extra, build)

    def _workspace(self, slot: str, key: tuple, dev, nbytes: Callable) -> tuple:
        """The float32 workspaces held in the workspace slot `slot` under `key`, one per byte count of nbytes() — which is asked, and the
        one entry replaced, only when the key is new."""
        if key not in getattr(self, slot):
            setattr(self, slot, {key: tuple(torch.empty(n // 4, device=dev, dtype=torch.float32) for n in nbytes())})
        return getattr(self, slot)[key]

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
        from . import _lib
        trunk, toks = self._trunk_parameters(), self._token_parameters()
        refuse_off_device("trunk_route", "device", (x, rel_pose16), trunk + toks, itertools.chain((x,), self.parameters()))
        lib, dev, call = _lib.api(), x.device, _lib.user_call
        BV, _, H, W = x.shape
        depths = (ctypes.c_int * 3)(*self.TRUNK_DEPTHS)
        grid = int(math.sqrt(toks[3].shape[1] - 1))

        def pack_tokens(table, src, out):                                      # the one pack entry that takes its arrays one by one
            pw, pb, cls, pos, sw, sb = map(_lib.ptr, src)
            call(lib.car_vit_tokens_pack, pw, pb, cls, pos, grid, sw, sb, gh, gw, _lib.ptr(out), _lib.stream())
        with torch.cuda.device(dev):
            packed = self._cached("_trunk_packed", trunk, (str(dev), self.TRUNK_DEPTHS), lambda: pack_parameters(
                trunk, dev, call(lib.car_trunk_packed_floats, depths),
                lambda table, src, out: call(lib.car_trunk_pack, table, len(src), depths, _lib.ptr(out), _lib.stream())))
            tpacked = self._cached("_tokens_packed", toks, (str(dev), gh, gw), lambda: pack_parameters(
                toks, dev, call(lib.car_vit_tokens_packed_floats, gh, gw), pack_tokens))
            work, twork = self._workspace("_trunk_work", (BV, H, W, str(dev)), dev, lambda: (
                call(lib.car_trunk_workspace_bytes, BV, H, W, depths), call(lib.car_vit_tokens_workspace_bytes, BV, gh, gw)))
            up = lambda v, k: -(-v // k)
            h4, w4, h8, w8, h16, w16 = up(H, 4), up(W, 4), up(H, 8), up(W, 8), up(H, 16), up(W, 16)
            if (h16, w16) != (gh, gw):
                raise ValueError(f"trunk_route = 'device': a {H}x{W} image gives {h16}x{w16} trunk features, not the {gh}x{gw} token grid")
            layer_1 = torch.empty(BV, h4, w4, 256, device=dev, dtype=torch.float32)
            layer_2 = torch.empty(BV, h8, w8, 512, device=dev, dtype=torch.float32)
            feat = torch.empty(BV, h16 * w16, 1024, device=dev, dtype=torch.float32)
            tok = torch.empty(BV, 1 + gh * gw, 768, device=dev, dtype=torch.float32)
            xc, pose = x.contiguous(), rel_pose16.contiguous()
            call(lib.car_trunk_forward, _lib.ptr(xc), BV, H, W, _lib.ptr(packed), depths, _lib.ptr(layer_1), _lib.ptr(layer_2), _lib.ptr(feat),
                 _lib.ptr(work), work.numel() * 4, _lib.stream())
            call(lib.car_vit_tokens, _lib.ptr(feat), BV, gh, gw, _lib.ptr(pose), _lib.ptr(tpacked), _lib.ptr(tok), _lib.ptr(twork),
                 twork.numel() * 4, _lib.stream())
        return layer_1.permute(0, 3, 1, 2), layer_2.permute(0, 3, 1, 2), tok      # NCHW views: torch's convolutions take channels_last

    def _vit_parameters(self) -> List[Tensor]:
        """The blocks' parameters in car_vit_pack's order (12 per block)."""
        names = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
                 "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")
        return [blk.get_parameter(n) for blk in self.pretrained.model.blocks for n in names]

    def _vit_workspace(self, lib, b: int, S: int, dim: int, dev) -> Tensor:
        return self._workspace("_vit_work", (b, S, str(dev)), dev, lambda: (lib.car_vit_workspace_bytes(b, S, dim),))[0]

    def _blocks_recorded_on_device(self, tok: Tensor, BV: int, T: int) -> dict:
        """The transformer stage where autograd records (vit_route = "device_train"): car_vit_blocks_train, with car_vit_blocks_backward
        as its backward.  tok [b, V T, dim] -> {tap: [BV, T, dim]}, each carrying the gradient back to tok and to the 144 block parameters."""
        params = self._vit_parameters()
        refuse_off_device("vit_route", self.vit_route, (tok,), params, None)    # this route has the backward
        outs = _VitBlocksTrain.apply(self, BV, T, tok, *params)
        return dict(zip(self.VIT_TAPS, outs))

    def _blocks_on_device(self, tok: Tensor, x: Tensor, BV: int, T: int) -> dict:
        """The transformer stage through car_vit_blocks: tok [b, V T, dim] (contiguous, overwritten) -> {tap: [BV, T, dim]}."""
        return self._blocks_inference(tok, x, BV, T, False)

    def _blocks_inference(self, tok: Tensor, x: Tensor, BV: int, T: int, recorded_elsewhere: bool) -> dict:
        """_blocks_on_device's body.  recorded_elsewhere (vit_route = "device_train" only): grad mode may be on, but neither tok nor a block
        parameter asks for a gradient, so nothing would flow through the blocks — the inference call is the whole of it."""
        from . import _lib
        params = self._vit_parameters()
        refuse_off_device("vit_route", self.vit_route, (tok,), params, None if recorded_elsewhere else itertools.chain((x,), self.parameters()),
                          inference="device")
        lib, dev, call = _lib.api(), tok.device, _lib.user_call
        b, S, dim = tok.shape
        depth = len(params) // 12
        with torch.cuda.device(dev):
            packed = self._cached("_vit_packed", params, (str(dev), dim, depth), lambda: pack_parameters(
                params, dev, call(lib.car_vit_packed_floats, dim, depth),
                lambda table, src, out: call(lib.car_vit_pack, table, len(src), dim, depth, _lib.ptr(out), _lib.stream())))
            work = self._vit_workspace(lib, b, S, dim, dev)
            outs = [torch.empty(BV, T, dim, device=dev, dtype=torch.float32) for _ in self.VIT_TAPS]
            call(lib.car_vit_blocks, _lib.ptr(tok), b, S, dim, _lib.ptr(packed), depth, (ctypes.c_int * len(outs))(*self.VIT_TAPS),
                 len(outs), (ctypes.c_void_p * len(outs))(*[t.data_ptr() for t in outs]), _lib.ptr(work), work.numel() * 4, _lib.stream())
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
        from . import _lib
        params = self._decoder_parameters()
        refuse_off_device("decoder_route", "device", (tap3, tap4, layer_1, layer_2), params, itertools.chain((x,), self.parameters()))
        lib, dev, call = _lib.api(), tap3.device, _lib.user_call
        BV = tap3.shape[0]
        with torch.cuda.device(dev):
            packed = self._cached("_decoder_packed", params, (str(dev),), lambda: pack_parameters(
                params, dev, call(lib.car_decoder_packed_floats),
                lambda table, src, out: call(lib.car_decoder_pack, table, len(src), _lib.ptr(out), _lib.stream())))
            work, = self._workspace("_decoder_work", (BV, gh, gw, str(dev)), dev, lambda: (call(lib.car_decoder_workspace_bytes, BV, gh, gw),))
            if tuple(layer_1.shape[-2:]) != (4 * gh, 4 * gw) or tuple(layer_2.shape[-2:]) != (2 * gh, 2 * gw):
                raise ValueError(f"decoder_route = 'device': stage ends of {tuple(layer_1.shape[-2:])} and {tuple(layer_2.shape[-2:])} are not 4 and 2 times "
                                 f"the {gh}x{gw} token grid")
            l1, l2 = layer_1.permute(0, 2, 3, 1).contiguous(), layer_2.permute(0, 2, 3, 1).contiguous()     # no copy behind trunk_route = 'device'
            t3, t4 = tap3.contiguous(), tap4.contiguous()
            path_2 = torch.empty(BV, 4 * gh, 4 * gw, 256, device=dev, dtype=torch.float32)
            path_1 = torch.empty(BV, 8 * gh, 8 * gw, 256, device=dev, dtype=torch.float32)
            call(lib.car_decoder_forward, _lib.ptr(t3), _lib.ptr(t4), _lib.ptr(l1), _lib.ptr(l2), BV, gh, gw, _lib.ptr(packed), _lib.ptr(path_2),
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
