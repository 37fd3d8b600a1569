"""Shared CLI of the eval / render entry points.  Flag names follow the reference's scripts
(eval_realestate10k.py:34-72, render_realestate10k_traj.py:37-82); configargparse is not installed here, so plain argparse.

Differences from the reference, all additive:
  --gpus N        shards the RAYS of every frame over N processes (RCCL all-gather of the tiles) instead of spawning N
                  identical replicas (eval_realestate10k.py:95-99);
  --synthetic     seeded synthetic stereo pair + feature pyramid (default when --data_root is absent: the datasets and the
                  DPT encoder weights are not available offline);
  --out_dir       where frames (PNG + NPY) and metrics are written;
  --lpips_weights VGG [LIN]   the caller's LPIPS weight files: with them the eval / render scripts report LPIPS too.
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parser(description: str) -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description=description)
    p.add_argument("--experiment_name", type=str, required=True)
    p.add_argument("--logging_root", type=str, default="logs")
    p.add_argument("--data_root", type=str, default=None, help="directory of scene directories (one *.npz of frames each)")
    p.add_argument("--pose_root", type=str, default=None,
                   help="directory of <scene>.txt camera files (RealEstate10K format); the train script takes the .mat pose table instead")
    p.add_argument("--checkpoint_path", type=str, default=None)
    p.add_argument("--batch_size", type=int, default=1)
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--views", type=int, default=2)
    p.add_argument("--model", type=str, default="midas_vit")
    p.add_argument("--img_sidelength", type=int, default=256)
    p.add_argument("--no_sample", action="store_true", default=False)
    p.add_argument("--no_latent_concat", action="store_true", default=False)
    p.add_argument("--no_multiview", action="store_true", default=False)
    p.add_argument("--no_high_freq", action="store_true", default=False)
    p.add_argument("--reconstruct", action="store_true", default=False)
    p.add_argument("--synthetic", action="store_true", default=False)
    p.add_argument("--with_encoder", action="store_true", default=False,
                   help="build the DPT encoder and run get_z on the context images even without a checkpoint (random weights)")
    p.add_argument("--n_frames", type=int, default=8, help="frames of the rendered trajectory")
    p.add_argument("--out_dir", type=str, default=None)
    p.add_argument("--cameras", choices=("host", "gpu", "device"), default="host",
                   help="where the camera matrices live and the 4x4 pose algebra runs: host = matrices stay on the CPU, the reference's "
                        "torch.inverse calls there (strict parity, no device sync; default); gpu = the whole input dict on the GPU as in the "
                        "reference's scripts, the engine downloads the matrices for the same host algebra (strict parity, one small sync per "
                        "new pose); device = car_pose_setup on the GPU (no host work per frame, last-ulp differences)")
    p.add_argument("--lpips_weights", type=str, nargs="+", default=None, metavar=("VGG", "LIN"),
                   help="report LPIPS (v0.1, net='vgg') computed on the device with these weight files: a torchvision VGG16 state dict and "
                        "the lpips package's vgg.pth, or one file holding lpips.LPIPS(net='vgg').state_dict().  Without it LPIPS is not reported "
                        "(no weights are shipped)")
    p.add_argument("--encoder_route", choices=("torch", "device", "device_train", "device_trunk", "device_full"), default="torch",
                   help="where get_z's encoder runs: torch = stock PyTorch (default); device = the transformer blocks on the library's own kernels "
                        "(car_vit_blocks: opt-in, inference only, float32; the rest of the encoder stays torch); device_trunk = the ResNetV2 trunk "
                        "and the token assembly as well (car_trunk_forward, car_vit_tokens; the read-out and the fusion stay torch); device_full = the read-out, the fusion, the image "
                        "normalisation and conv_map as well (car_decoder_forward, car_normalize_rgb, car_conv7x7_pad3: no torch operator is left in get_z but "
                        "the relative pose's 4x4 algebra).  Read only where the encoder "
                        "is built (a checkpoint or --with_encoder); the train script applies these to its validation pass only, because a forward "
                        "that autograd records refuses them; device_train = the transformer blocks with a backward (car_vit_blocks_train, "
                        "car_vit_blocks_backward): the one value the train script applies to its training forward; under no_grad it is device")
    p.add_argument("--port", type=int, default=1492)          # the reference rendezvous port (eval_realestate10k.py:97)
    return p


def add_precision(p):
    """--precision of the inference scripts (render / eval): the arithmetic of the fused per-sample kernel (model.render_precision)."""
    p.add_argument("--precision", choices=("fp32", "fp16"), default="fp32",
                   help="fp32 = 1e-4 parity with the reference (default); fp16 = the opt-in reduced precision of the two-view one-call route "
                        "(one fp16 product per term in the fused per-sample kernel, ~25 %% faster frames, errors far below an 8-bit frame's "
                        "step; DESIGN.md 4.11).  Configurations off that route refuse fp16 instead of falling back")
    return p


def build_model(opt, device, with_encoder=None):
    """The renderer; with a checkpoint (or --with_encoder) the multi-view DPT encoder is built too, so that ``get_z`` runs on the
    context images.  Loading follows the reference (strict unless --reconstruct, eval_realestate10k.py:110-118) and FAILS on keys that
    do not match instead of silently leaving layers at their initial values."""
    import torch
    from cross_attention_renderer_amd import synthetic
    from cross_attention_renderer_amd.models import CrossAttentionRenderer
    torch.manual_seed(0)
    if with_encoder is None:
        with_encoder = bool(opt.checkpoint_path) or getattr(opt, "with_encoder", False)
    model = CrossAttentionRenderer(no_sample=opt.no_sample, no_latent_concat=opt.no_latent_concat,
                                   no_multiview=opt.no_multiview, no_high_freq=opt.no_high_freq, model=opt.model,
                                   n_view=opt.views, with_encoder=with_encoder).eval()
    if opt.checkpoint_path:
        state = torch.load(opt.checkpoint_path, map_location="cpu")["model"]
        res = model.load_state_dict(state, strict=False)
        bad = [k for k in res.missing_keys if not opt.reconstruct] + list(res.unexpected_keys)
        if bad:
            raise SystemExit(f"checkpoint {opt.checkpoint_path} does not match the model: {len(res.missing_keys)} missing, "
                             f"{len(res.unexpected_keys)} unexpected keys, e.g. {bad[:6]}")
    else:
        with torch.no_grad():                            # un-trained weights: fc_1 is zero-initialised otherwise (resnet_block_fc.py:39)
            g = torch.Generator().manual_seed(0)
            for n_, p_ in model.named_parameters():
                if not n_.startswith("encoder."):
                    p_.add_(0.02 * torch.randn(p_.shape, generator=g))
    model.H = model.W = opt.img_sidelength
    model.pose_route = "device" if getattr(opt, "cameras", "host") == "device" else "host"
    model.render_precision = getattr(opt, "precision", "fp32")
    if with_encoder:                                     # a renderer-only module never calls get_z: the flag has nothing to switch there
        model.encoder_route = getattr(opt, "encoder_route", "torch")
    return model.to(device)


def lpips_weights(opt):
    """The weights named by --lpips_weights (harness.load_lpips_weights), or None without the option."""
    paths = getattr(opt, "lpips_weights", None)
    if not paths:
        return None
    if len(paths) > 2:
        raise SystemExit("--lpips_weights takes one file (the lpips package's state dict) or two (VGG16 state dict, lin weights)")
    from cross_attention_renderer_amd import harness
    return harness.load_lpips_weights(paths[0], paths[1] if len(paths) == 2 else None)


def spawn(fn, opt):
    """One process per GPU, NCCL(=RCCL) process group over tcp://127.0.0.1:<port> as in the reference scripts."""
    import torch.multiprocessing as mp
    if opt.gpus > 1:
        mp.spawn(fn, nprocs=opt.gpus, args=(opt,), join=True)
    else:
        fn(0, opt)


def init_rank(rank, opt):
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(rank)
    if opt.gpus > 1:
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{opt.port}", world_size=opt.gpus, rank=rank)
    return torch.device("cuda", rank)
