"""``CrossAttentionRenderer`` — the drop-in module boundary (reference models.py:42-626).

Same constructor signature, same parameter names/shapes (so a reference checkpoint loads with
``load_state_dict``), same ``get_z`` / ``forward(input, z=None, val=False, debug=False) -> dict`` contract and
the same output-dict keys.  Underneath, ``forward`` runs hand-written HIP kernels for gfx950 through the
C-ABI library ``libcar_hip.so`` (``include/car_hip.h``); there is **no** PyTorch or CPU fallback on the render
path: if the library is missing or the tensors are not on a ROCm device, ``forward`` raises.

What stays stock PyTorch here is only what the reference also leaves to the framework outside the hot loop:
parameter storage, ``get_z`` (image encoder + ``conv_map``, once per stereo pair) and output-dict assembly.
"""
from __future__ import annotations

import itertools
from typing import Dict, List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .encoder import MultiViewDPTEncoder, refuse_off_device

Tensor = torch.Tensor


class ResnetBlockFC(nn.Module):
    """Parameter holder mirroring resnet_block_fc.py:10-62 (fc_0, fc_1; fc_1.weight zero-initialised)."""

    def __init__(self, size: int):
        super().__init__()
        self.fc_0 = nn.Linear(size, size)
        self.fc_1 = nn.Linear(size, size)
        nn.init.constant_(self.fc_0.bias, 0.0)
        nn.init.kaiming_normal_(self.fc_0.weight, a=0, mode="fan_in")
        nn.init.constant_(self.fc_1.bias, 0.0)
        nn.init.zeros_(self.fc_1.weight)


class ResnetFC(nn.Module):
    """Parameter holder mirroring resnet_block_fc.py:65-130 (lin_in, lin_out, blocks.i, lin_z.i)."""

    def __init__(self, d_in: int, d_out: int, n_blocks: int, d_latent: int, d_hidden: int):
        super().__init__()
        self.d_in, self.d_out, self.n_blocks, self.d_latent, self.d_hidden = d_in, d_out, n_blocks, d_latent, d_hidden
        self.lin_in = nn.Linear(d_in, d_hidden)
        self.lin_out = nn.Linear(d_hidden, d_out)
        self.blocks = nn.ModuleList([ResnetBlockFC(d_hidden) for _ in range(n_blocks)])
        self.lin_z = nn.ModuleList([nn.Linear(d_latent, d_hidden) for _ in range(n_blocks)])
        for lin in [self.lin_in, self.lin_out, *self.lin_z]:
            nn.init.constant_(lin.bias, 0.0)
            nn.init.kaiming_normal_(lin.weight, a=0, mode="fan_in")


class EncoderNotBuilt(nn.Module):
    """Placeholder used when the module is built with ``with_encoder=False`` (renderer-only use: tests, benchmarks and hosts that
    feed precomputed feature maps through ``forward(input, z=z)``) or for the reference's other ``model=`` strings, whose encoders
    (ResNet34 ``SpatialEncoder``, MiDaS-small, the broken ``UNetEncoder``; models.py:63-81, 97-99) are not built here.  Assign any
    module with ``forward(rgb, rel_pose16, n_view) -> [path_2, path_1]`` to ``renderer.encoder`` to make ``get_z`` work.
    """

    def forward(self, *a, **k):
        raise NotImplementedError(
            "image encoder not built: construct CrossAttentionRenderer(model='midas_vit', with_encoder=True), pass precomputed "
            "feature maps via forward(input, z=z), or assign renderer.encoder = <module returning [path_2 (256@H/4), path_1 (256@H/2)]>")


def _feature_dim(model: str) -> int:
    """Channel count of the concatenated feature pyramid (models.py:63-99)."""
    if model in ("resnet", "midas"):
        return 512
    if model == "midas_vit":
        return 512 + 64
    return 32


class CrossAttentionRenderer(nn.Module):
    def __init__(self, no_sample=False, no_latent_concat=False, no_multiview=False, no_high_freq=False,
                 model="midas_vit", uv=None, repeat_attention=True, n_view=1, npoints=64,
                 num_hidden_units_phi=128, encoder: Optional[nn.Module] = None, with_encoder: bool = True):
        super().__init__()
        self.n_view = n_view
        self.npoints = 64 if n_view in (1, 2) else 48
        if npoints:
            self.npoints = npoints                          # models.py:53-54 (default 64 overrides 48)
        self.repeat_attention = repeat_attention
        self.no_sample = no_sample
        self.no_latent_concat = no_latent_concat
        self.no_multiview = no_multiview
        self.no_high_freq = no_high_freq
        self.model = model
        self.num_hidden_units_phi = num_hidden_units_phi

        # reference: DPTDepthModel(backbone="vitb_rn50_384") with its stem convolution replaced (models.py:82-94).  ``encoder=`` and
        # ``with_encoder=`` are additions of this repo: the 123 M-parameter encoder is only needed by get_z.
        if encoder is not None:
            self.encoder = encoder
        elif with_encoder and model == "midas_vit":
            self.encoder = MultiViewDPTEncoder()
        else:
            self.encoder = EncoderNotBuilt()
        self.latent_dim = _feature_dim(model)
        self.feature_dim = self.latent_dim
        if model == "midas_vit":
            self.conv_map = nn.Conv2d(3, 64, kernel_size=7, stride=1, padding=3)

        if self.n_view > 1 and not self.no_latent_concat:
            self.query_encode_latent = nn.Conv2d(self.latent_dim + 3, self.latent_dim, 1)
            self.query_encode_latent_2 = nn.Conv2d(self.latent_dim, self.latent_dim // 2, 1)
            self.latent_dim = self.latent_dim // 2
            self.update_val_merge = nn.Conv2d(self.latent_dim * 2 + 6, self.latent_dim, 1)
        elif self.no_latent_concat:
            self.feature_map = nn.Conv2d(self.latent_dim, self.latent_dim // 2, 1)
        else:
            self.update_val_merge = nn.Conv2d(self.latent_dim + 6, self.latent_dim, 1)

        hidden_dim = 128
        self.hidden_dim = hidden_dim
        if not self.no_latent_concat:
            self.latent_value = nn.Conv2d(self.latent_dim * self.n_view, self.latent_dim, 1)
            self.key_map = nn.Conv2d(self.latent_dim * self.n_view, hidden_dim, 1)
        else:
            self.latent_value = nn.Conv2d(self.latent_dim, self.latent_dim, 1)
            self.key_map = nn.Conv2d(self.latent_dim, hidden_dim, 1)
        self.key_map_2 = nn.Conv2d(hidden_dim, hidden_dim, 1)

        self.query_embed = nn.Conv2d(16, hidden_dim, 1)
        self.query_embed_2 = nn.Conv2d(hidden_dim, hidden_dim, 1)
        # declared by the reference but unused in forward; kept so checkpoints load
        self.latent_avg_query = nn.Conv2d(9 + 16, hidden_dim, 1)
        self.latent_avg_query_2 = nn.Conv2d(hidden_dim, hidden_dim, 1)
        self.latent_avg_key = nn.Conv2d(self.latent_dim, hidden_dim, 1)
        self.latent_avg_key_2 = nn.Conv2d(hidden_dim, hidden_dim, 1)
        self.query_repeat_embed = nn.Conv2d(16 + 128, hidden_dim, 1)
        self.query_repeat_embed_2 = nn.Conv2d(hidden_dim, hidden_dim, 1)
        self.latent_avg_repeat_query = nn.Conv2d(9 + 16 + 128, hidden_dim, 1)
        self.latent_avg_repeat_query_2 = nn.Conv2d(hidden_dim, hidden_dim, 1)
        self.encode_latent = nn.Conv1d(self.latent_dim, 128, 1)

        self.phi = ResnetFC(self.n_view * 9, n_blocks=3, d_out=3, d_latent=self.latent_dim * self.n_view,
                            d_hidden=self.num_hidden_units_phi)
        self._engine = None
        # where forward's 4x4 pose algebra runs (engine._poses): "host" = the reference's torch.inverse on the CPU wherever the camera
        # tensors live (strict parity, the default); "device" = car_pose_setup on the GPU when the cameras are there (opt-in)
        self.pose_route = "host"
        # arithmetic of the inference forward's fused per-sample kernel: "fp32" (the default, 1e-4 parity with the reference) or the opt-in
        # "fp16" (one fp16 product per term; preview frames and trajectory videos — DESIGN.md 4.11).  "fp16" exists on the one-call route
        # only (two views, midas_vit widths, a common lattice): any other forward raises instead of falling back; training refuses it
        self.render_precision = "fp32"

    # -> (trunk_route, vit_route, decoder_route)
    ENCODER_ROUTES = {"torch": ("torch", "torch", "torch"), "device": ("torch", "device", "torch"), "device_trunk": ("device", "device", "torch"),
                      "device_full": ("device", "device", "device"), "device_train": ("torch", "device_train", "torch")}

    @property
    def encoder_route(self) -> str:
        """Where get_z's encoder runs: "torch" (the default), the opt-in "device" (the transformer blocks alone: car_vit_blocks,
        include/car_encoder.h), the opt-in "device_trunk" (the ResNetV2 trunk and the token assembly as well: car_trunk_forward and
        car_vit_tokens, include/car_trunk.h) or the opt-in "device_full" (the read-out, the re-assembly and the fusion too:
        car_decoder_forward, include/car_decoder.h — and get_z then also normalises the images and runs conv_map through car_normalize_rgb
        and car_conv7x7_pad3, so that only the 4x4 algebra of the relative pose is left to torch), or the opt-in "device_train" (the
        blocks alone, as "device" — and the same call under no_grad — but a forward that autograd records runs car_vit_blocks_train and
        trains through car_vit_blocks_backward, include/car_encoder_train.h; the trunk and the decoder stay torch autograd).  The other device routes are inference only,
        float32 on a CUDA device — get_z raises on anything else instead of falling back; the read-out, the fusion and conv_map are torch on
        every route but "device_full".  The value lives on the encoder (MultiViewDPTEncoder.trunk_route, vit_route and decoder_route; a
        combination set there that has no name here is returned as the pair (trunk_route, vit_route) while the decoder is on torch, as the
        triple (trunk_route, vit_route, decoder_route) otherwise); an encoder without the switches — none built, or a caller's own module —
        has the "torch" route only."""
        triple = tuple(getattr(self.encoder, a, "torch") for a in ("trunk_route", "vit_route", "decoder_route"))
        return next((name for name, p in self.ENCODER_ROUTES.items() if p == triple), triple[:2] if triple[2] == "torch" else triple)

    @encoder_route.setter
    def encoder_route(self, value: str) -> None:
        if value not in self.ENCODER_ROUTES:
            raise ValueError("encoder_route must be 'torch' or 'device' (the blocks alone), 'device_train' (the blocks, with a backward), "
                             f"'device_trunk' or 'device_full' (got {value!r})")
        trunk, vit, decoder = self.ENCODER_ROUTES[value]
        if hasattr(self.encoder, "vit_route"):
            self.encoder.vit_route = vit
            for attr, route in (("trunk_route", trunk), ("decoder_route", decoder)):
                if hasattr(self.encoder, attr):
                    setattr(self.encoder, attr, route)
                elif route != "torch":
                    raise ValueError(f"encoder_route = {value!r} needs the built-in MultiViewDPTEncoder: {type(self.encoder).__name__} has no {attr}")
        elif value != "torch":
            raise ValueError(f"encoder_route = {value!r} needs the built-in MultiViewDPTEncoder (model='midas_vit', with_encoder=True): "
                             f"{type(self.encoder).__name__} has no vit_route")

    @property
    def render_precision(self) -> str:
        return self._render_precision

    @render_precision.setter
    def render_precision(self, value: str) -> None:
        if value not in ("fp32", "fp16"):
            raise ValueError(f"render_precision must be 'fp32' or 'fp16' (got {value!r})")
        self._render_precision = value

    def train(self, mode: bool = True):
        """Leaving train() mode for eval() — the validation pass between optimizer steps (summaries.render_full) — sets aside what the
        engine built from the parameters and renders from empty caches: torch's fused optimizers update parameters without advancing
        ``_version``, which the engine's cache keys rely on (engine.RenderEngine.park_parameter_caches).  Returning to train() mode puts
        the training loop's caches back as they were.  A module that was never in train() mode is not touched.  The encoder's packed
        transformer blocks (encoder_route = "device") have the same problem in the same pass and are dropped in the same transition: the
        next eval() get_z packs the parameters as they are then."""
        engine = getattr(self, "_engine", None)
        if self.training and not mode and hasattr(getattr(self, "encoder", None), "drop_device_caches"):
            self.encoder.drop_device_caches()
        if engine is not None and self.training and not mode:
            self._parked_caches = engine.park_parameter_caches()
        elif engine is not None and not self.training and mode and getattr(self, "_parked_caches", None) is not None:
            engine.restore_parameter_caches(self._parked_caches)
            self._parked_caches = None
        return super().train(mode)

    # ------------------------------------------------------------------------------------------
    def get_z(self, input, val=False) -> List[Tensor]:
        """Feature pyramid of the context views, NCHW (models.py:148-188).  Stock PyTorch by default; with encoder_route = "device" the
        encoder's transformer blocks run on the library's kernels, with "device_trunk" its trunk and token assembly too, with "device_full"
        everything but the relative pose's 4x4 algebra (inference only)."""
        rgb = input["context"]["rgb"]
        cam2world = input["context"]["cam2world"]
        rel_cam2world = torch.matmul(torch.inverse(cam2world[:, :1]), cam2world)
        on_device = self.model == "midas_vit" and self.encoder_route == "device_full"
        if on_device:
            rgb_cl = torch.flatten(rgb, 0, 1)                           # [BV, H, W, 3]: the layout car_normalize_rgb reads
            self.H, self.W = rgb_cl.shape[1], rgb_cl.shape[2]
            self._refuse_off_device(rgb_cl, [*self.encoder.parameters(), *self.conv_map.parameters()])
            rgb = self._normalize_on_device(rgb_cl)
            pose16 = rel_cam2world.reshape(-1, 16).to(rgb.device)
            if self.no_multiview:
                pose16 = torch.zeros_like(pose16)
            return list(self.encoder.forward(rgb, pose16, self.n_view)) + [self._conv_map_on_device(rgb)]
        rgb = torch.flatten(rgb, 0, 1).permute(0, -1, 1, 2)
        self.H, self.W = rgb.shape[-2], rgb.shape[-1]
        if self.model in ("resnet", "midas", "midas_vit"):
            rgb = (rgb + 1) / 2.0
            mean = rgb.new_tensor([0.485, 0.456, 0.406])[None, :, None, None]
            std = rgb.new_tensor([0.229, 0.224, 0.225])[None, :, None, None]
            rgb = (rgb - mean) / std
        pose16 = rel_cam2world.reshape(-1, 16).to(rgb.device)       # the cameras may live on the host (engine._poses)
        if self.no_multiview:
            pose16 = torch.zeros_like(pose16)
        z = list(self.encoder.forward(rgb, pose16, self.n_view))
        if self.model in ("midas", "midas_vit"):
            z_conv = self.conv_map(rgb)
            if self.no_high_freq:
                z_conv = torch.zeros_like(z_conv)
            z = z + [z_conv]
        return z

    def _refuse_off_device(self, t: Tensor, params) -> None:
        """encoder_route = "device_full" makes the refusals of the encoder's own switches for get_z's two lines around the encoder."""
        refuse_off_device("encoder_route", "device_full", (t,), params, itertools.chain((t,), params), model="the model", call="call get_z")

    def _normalize_on_device(self, rgb_cl: Tensor) -> Tensor:
        """get_z's normalisation through car_normalize_rgb: [BV, H, W, 3] in [-1, 1] -> [BV, 3, H, W]."""
        from . import _lib
        self._refuse_off_device(rgb_cl, ())
        lib, (n, H, W, _) = _lib.api(), rgb_cl.shape
        with torch.cuda.device(rgb_cl.device):
            src, out = rgb_cl.contiguous(), torch.empty(n, 3, H, W, device=rgb_cl.device, dtype=torch.float32)
            _lib.user_call(lib.car_normalize_rgb, _lib.ptr(src), n, H, W, _lib.ptr(out), _lib.stream())
        return out

    def _conv_map_on_device(self, x: Tensor) -> Tensor:
        """conv_map through car_conv7x7_pad3: x [BV, 3, H, W] -> an NCHW view of the channel-last [BV, H, W, 64] (zeros under no_high_freq)."""
        from . import _lib
        w, b = self.conv_map.weight, self.conv_map.bias
        self._refuse_off_device(x, (w, b))
        lib, (n, _, H, W) = _lib.api(), x.shape
        if self.no_high_freq:
            return torch.zeros(n, H, W, 64, device=x.device, dtype=torch.float32).permute(0, 3, 1, 2)
        with torch.cuda.device(x.device):
            out = torch.empty(n, H, W, 64, device=x.device, dtype=torch.float32)
            _lib.user_call(lib.car_conv7x7_pad3, _lib.ptr(x), n, H, W, _lib.ptr(w.detach().contiguous()), _lib.ptr(b.detach().contiguous()), _lib.ptr(out),
                           _lib.stream())
        return out.permute(0, 3, 1, 2)

    # ------------------------------------------------------------------------------------------
    def forward(self, input, z=None, val=False, debug=False) -> Dict[str, Tensor]:
        """Render the query rays (models.py:190-626) on the HIP engine.  ``input`` is not mutated."""
        from .engine import RenderEngine          # deferred: importing the package must work without the .so
        if self.training and torch.is_grad_enabled() and not debug and (
                any(p.requires_grad for p in self.parameters()) or (z is not None and any(t.requires_grad for t in z))):
            # the reference's training loop calls model(model_input) on a module in train() mode under autograd (training.py:92): the same
            # call here is the forward with gradients (training.render_train: HIP forward and backward); eval() / no_grad() callers — the
            # render and eval scripts — take the inference engine below
            from .training import render_train
            return render_train(self, input, z)
        if z is None:
            z = self.get_z(input)
        elif not hasattr(self, "H"):
            # the reference requires get_z to have run (models.py:162); recover H, W from the RGB shape
            self.H, self.W = input["context"]["rgb"].shape[2:4]
        if self._engine is None:
            self._engine = RenderEngine(self)
        return self._engine.render(input, z, debug=debug)


    def prefetch_pair(self, z) -> bool:
        """Eval-loop hook (not in the reference, whose loop pays nothing per pair): announce the NEXT stereo pair's pyramid ``z`` — the list
        ``get_z`` returned for the next batch — before rendering the current one.  Its per-pair set-up (channel-last copies, the first
        point-MLP layer per texel, the common lattice: ``car_project_maps``, 1.3 ms at 256 x 256) then runs on a side stream beside the
        current frame's kernels instead of in front of the next frame.  Optional: ``forward`` computes the same thing itself when it was not
        announced.  Returns whether anything was started (engine.RenderEngine.prefetch)."""
        if self._engine is None:
            return False
        return self._engine.prefetch(list(z))


def renderer_param_shapes(model="midas_vit", n_view=2, no_latent_concat=False) -> Dict[str, tuple]:
    """name -> shape of every renderer parameter except the image encoder's."""
    m = CrossAttentionRenderer(model=model, n_view=n_view, no_latent_concat=no_latent_concat, with_encoder=False)
    return {k: tuple(v.shape) for k, v in m.state_dict().items() if not k.startswith("encoder.")}
