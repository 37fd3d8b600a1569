"""Training entry point (mirrors reference experiment_scripts/train_realestate10k.py + training.py:46-246).

    python experiment_scripts/train_realestate10k.py --experiment_name demo --views 2 --batch_size 12 --synthetic [--gpus N] [--max_steps K]
    python experiment_scripts/train_realestate10k.py --experiment_name demo --views 2 --data_root DIR --pose_root FILE.mat [--no_data_aug] [--num_workers N]

The reference's loop, with ``training.render_train`` (HIP forward + HIP backward, csrc/car_backward.hip) in the place of
``model(model_input)``: Adam(lr, betas=(0.99, 0.999)) (train_realestate10k.py:93), 192 random query rays per scene (query_sparsity,
train_realestate10k.py:78), L1 image loss (loss_functions.image_loss; --depth adds the reference's per-patch depth-variance term on 32 x 32
pixel patches, loss_functions.py:112-127, and samples the rays as such patches: --query_sparsity must then be a multiple of 1024; --lpips
adds the reference's second-stage term, loss_functions.py:102-118: lpips_coeff x LPIPS_vgg(gt, pred) of the same 32 x 32 patches, masked
per patch, its forward and backward on the device — harness.lpips_loss, csrc/car_lpips.hip — with the weight files named by
--lpips_weights, since none are shipped),
gradient clipping at norm 1 (training.py:130-134), parameters broadcast from rank 0 and gradients all-reduced when --gpus > 1
(train_realestate10k.py:60-62, training.py:21-28: one process per GPU over RCCL), checkpoints ``{'model', 'optimizer'}`` as
``checkpoints/model_current.pth`` / ``model_final.pth`` (training.py:82-84, 244-246) that the eval / render scripts load.

Data.  With --data_root DIR --pose_root FILE.mat the script trains on the RealEstate10K reader (dataio.RealEstate10k: the reference's frame
draw, augmentation unless --no_data_aug, and ray sampling, train_realestate10k.py:74-81) through dataio.TrainLoader: --num_workers threads
read the scenes, the raw uint8 frames of a batch go to the device in one copy and the resize / flip / crop chain runs there
(csrc/car_frames.hip).  The encoder is built and the pyramid comes from ``get_z`` under autograd; the L1 loss uses the batch's rgb;
--lpips and --depth work on the reader's 1024 rays per scene and its per-scene mask (1 where the rays are one 32 x 32 patch), exactly as
loss_functions.py:102-129, so --depth needs --lpips there (the reader only yields patches under lpips); with --gpus N every rank seeds
its loader by its rank.
Without --data_root scenes are synthetic (--synthetic, the default: seeded stereo pairs with a smooth random target image per scene;
every step draws new rays).  There the encoder trains when the model is built with it (--with_encoder: the pyramid then comes from
``get_z`` under autograd); otherwise the pyramid itself is a leaf that receives gradients, standing in for the encoder's output.

Summaries and validation (training.py:95-117, 142-235; cross_attention_renderer_amd/summaries.py), all opt-in — without these flags the loop
is the one above.  --summaries logs, on rank 0 and at every step, each loss under the reference's name (img_loss, lpips_loss, depth_loss),
total_train_loss and total_at_entropy (one small kernel on the detached at_wt of the training forward) to
<logging_root>/<experiment>/summaries; the values stay on the device and the log is flushed at summary steps only, so the loop stays
sync-free in between.  --val_root DIR --val_pose_root FILE.mat [--val_batch_size 8] run the reference's validation pass at every summary
step on rank 0: one shuffled batch of full images (RealEstate10k(augment=False, query_sparsity=None)) rendered in eval() mode under
no_grad through summaries.render_full, the losses with val=True (no depth term; LPIPS over the full image's rays reshaped (-1, 32, 32, 3),
unmasked) as val_<loss>, and the five image panels of summaries.img_summaries under the prefix val_.  With synthetic scenes --summaries
validates on one synthetic batch of --val_batch_size scenes with the full pixel grid (--val_batch_size 0: no validation pass).  Validation enters no collective: the other ranks go
on to their next all-reduce and wait there, as in the reference.  --iters_til_ckpt N writes checkpoints/model_epoch_%04d_iter_%06d.pth
every N steps (training.py:233-235; not at step 0, where the reference stores the untrained model)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import common  # noqa: E402


def _parser():
    p = common.parser(__doc__)
    p.add_argument("--lr", type=float, default=5e-5)
    p.add_argument("--l2_coeff", type=float, default=0.05)
    p.add_argument("--depth", action="store_true", default=False)
    p.add_argument("--lpips", action="store_true", default=False,
                   help="add lpips_coeff x LPIPS (v0.1, net='vgg') of the 32 x 32 ray patches to the loss; needs --lpips_weights")
    p.add_argument("--lpips_coeff", type=float, default=0.1)            # loss_functions.py:118 (its comment: 0.2 for realestate)
    p.add_argument("--max_steps", type=int, default=20)
    p.add_argument("--steps_til_summary", type=int, default=10)
    p.add_argument("--query_sparsity", type=int, default=192)
    p.add_argument("--no_data_aug", action="store_true", default=False, help="--data_root: read the frames without flip / crop augmentation")
    p.add_argument("--num_workers", type=int, default=8, help="--data_root: reader threads (capped at 16)")
    p.add_argument("--replay_batch", action="store_true", default=False,
                   help="--data_root: train on the first batch over and over (tools/train_loader_timing.py: the step without the data wait)")
    p.add_argument("--summaries", action="store_true", default=False,
                   help="log the per-step scalars (losses, total_train_loss, total_at_entropy) to <logging_root>/<experiment>/summaries; with "
                        "synthetic scenes also validate on a synthetic batch at every summary step")
    p.add_argument("--val_root", type=str, default=None, help="validation scenes (as --data_root): run the validation pass at every summary step")
    p.add_argument("--val_pose_root", type=str, default=None, help="the validation scenes' .mat pose table")
    p.add_argument("--val_batch_size", type=int, default=8, help="scenes of a validation batch; 0 with synthetic scenes: --summaries without a validation pass")
    p.add_argument("--iters_til_ckpt", type=int, default=10000, help="write checkpoints/model_epoch_%%04d_iter_%%06d.pth every N steps")
    p.set_defaults(batch_size=12, synthetic=True)
    return p


def _smooth_image(uv, coef, H):
    """The synthetic target: low-frequency colours of the pixel coordinates ``uv`` (b, R, 2), one coefficient set (b, 3, 4) per scene."""
    import torch
    u = uv / (H - 1) * 3.14159
    feats = torch.stack([torch.sin(u[..., 0]), torch.cos(u[..., 1]), torch.sin(u[..., 0] + u[..., 1]), torch.ones_like(u[..., 0])], dim=-1)
    return torch.tanh(torch.einsum("brk,bck->brc", feats, coef))


def _validation_batches(opt, model, dev):
    """An endless iterator of validation batches ``(model_input, gt, z or None)`` with the full image's rays, on the device.  ``z`` is the
    stand-in pyramid when the model has no encoder (synthetic scenes), None when ``get_z`` provides it."""
    import torch
    from cross_attention_renderer_amd import harness, synthetic
    vb, H = opt.val_batch_size, opt.img_sidelength
    if opt.val_root:
        from cross_attention_renderer_amd import dataio
        ds = dataio.RealEstate10k(opt.val_root, opt.val_pose_root, num_ctxt_views=opt.views, num_query_views=1, query_sparsity=None,
                                  augment=False, lpips=opt.lpips)
        loader = dataio.TrainLoader(ds, batch_size=vb, seed=4242, num_workers=min(opt.num_workers, 4), device=dev, cameras=opt.cameras)
        if len(loader) == 0:
            raise SystemExit(f"--val_root {opt.val_root}: {len(ds)} scenes do not fill one batch of {vb}")
        while True:                                               # shuffled anew every epoch; one batch is taken per validation pass
            for inp, gt in loader:
                yield inp, gt, None
    # synthetic: one fixed batch — seeded scenes, smooth random colours for the context views and the target
    g = torch.Generator().manual_seed(977)
    base = harness.to_device(synthetic.stereo_scene(H, b=vb, seed=905, n_view=opt.views), dev, opt.cameras)
    grid = synthetic.pixel_grid(H, H).to(dev)
    coef = (torch.rand(vb, 1 + opt.views, 3, 4, generator=g) * 2 - 1).to(dev)
    uv = grid[None].expand(vb, H * H, 2)
    rgb = _smooth_image(uv, coef[:, 0], H)[:, None]                                                         # (vb, 1, H * H, 3)
    ctx = torch.stack([_smooth_image(uv, coef[:, 1 + v], H).view(vb, H, H, 3) for v in range(opt.views)], dim=1)
    inp = {"context": dict(base["context"], rgb=ctx), "query": dict(base["query"], rgb=rgb)}
    gt = {"rgb": rgb}
    z = None
    if model.encoder.__class__.__name__ == "EncoderNotBuilt":
        z = [t.to(dev) for t in synthetic.feature_maps(vb, opt.views, H, seed=907)]
    while True:
        yield inp, gt, z


def _train_route(opt):
    """The encoder route of the training forward: --encoder_route device_train trains through the blocks' device backward; every other
    device value is inference only and holds for the validation pass alone."""
    return "device_train" if getattr(opt, "encoder_route", "torch") == "device_train" else "torch"


def _validate(opt, model, batch, log, step, lpips_w):
    """One validation pass (training.py:146-231): eval(), no_grad, get_z once, the chunked full-image render, the losses with val=True, the
    val_ scalars and panels, train().  Nothing here waits for the device but the PNG writes.  --encoder_route holds for this pass alone
    (device_train excepted, which the training forward runs too): the training forward records get_z under autograd, which the other
    device routes refuse, so train() keeps the torch encoder for them."""
    import torch
    from cross_attention_renderer_amd import harness, summaries
    inp, gt, z = batch
    model.eval()
    try:
        if z is None:
            model.encoder_route = getattr(opt, "encoder_route", "torch")
        with torch.no_grad():
            if z is None:
                z = model.get_z(inp)
            out = summaries.render_full(model, inp, z, chunk_rays=harness.CHUNK_RAYS)
            val = {"img_loss": (gt["rgb"] - out["rgb"]).abs().mean()}                                       # loss_functions.image_loss
            if opt.lpips:                                         # loss_functions.py:102-118 on the full image: no mask fits its patches
                gt_p, pred_p = gt["rgb"].reshape(-1, 32, 32, 3).contiguous(), out["rgb"].reshape(-1, 32, 32, 3).contiguous()
                val["lpips_loss"] = opt.lpips_coeff * harness.lpips_loss(gt_p, pred_p, lpips_w).mean()
            for name, value in val.items():                       # val=True skips the depth term (loss_functions.py:120)
                log.add_scalar("val_" + name, value, step)
            summaries.img_summaries(model, inp, gt, {}, out, log, step, "val_", img_shape=(model.H, model.W), n_view=opt.views)
    finally:
        model.encoder_route = _train_route(opt)
        model.train()


def train(rank, opt):
    import torch
    import torch.distributed as dist
    from cross_attention_renderer_amd import harness, synthetic
    from cross_attention_renderer_amd import training
    from cross_attention_renderer_amd.training import average_gradients, render_train
    dev = common.init_rank(rank, opt)
    H, b, R = opt.img_sidelength, opt.batch_size, opt.query_sparsity
    real = bool(opt.data_root)                                    # the RealEstate10K reader; otherwise synthetic scenes, as before
    model = common.build_model(opt, dev, with_encoder=True if real else None).train()
    if model.encoder.__class__.__name__ != "EncoderNotBuilt":     # the training forward's get_z is recorded by autograd: torch, or the blocks'
        model.encoder_route = _train_route(opt)                   # recorded device route; _validate applies the other values of --encoder_route
    params = [p for p in model.parameters() if p.requires_grad]
    if opt.gpus > 1:                                              # sync_model (train_realestate10k.py:60-62)
        for p in params:
            dist.broadcast(p.data, 0)
    g = torch.Generator().manual_seed(1234 + rank)                 # every rank shuffles on its own (train_realestate10k.py:80-81)
    batches = None
    if real:
        from cross_attention_renderer_amd import dataio
        ds = dataio.RealEstate10k(opt.data_root, opt.pose_root, num_ctxt_views=opt.views, num_query_views=1, query_sparsity=R,
                                  augment=not opt.no_data_aug, lpips=opt.lpips)
        loader = dataio.TrainLoader(ds, batch_size=b, seed=1234 + rank, num_workers=opt.num_workers, device=dev, cameras=opt.cameras)
        if len(loader) == 0:
            raise SystemExit(f"--data_root {opt.data_root}: {len(ds)} scenes do not fill one batch of {b}")
        if opt.lpips:
            R = dataio.LPIPS_RAYS                                 # the reader's sampling under lpips: 1024 rays per scene, patch or not
        if rank == 0:
            print(f"data: RealEstate10K reader on {opt.data_root} ({len(ds)} scenes, augment {'off' if opt.no_data_aug else 'on'}, "
                  f"{loader.num_workers} reader threads, pixel chain on the device)", flush=True)

        def forever():                                            # epoch after epoch, each shuffled anew
            if opt.replay_batch:                                  # measurement: the step without any wait for data
                epoch = iter(loader)
                first = next(epoch)
                epoch.close()                                     # stops the reader's threads now, not when the generator is collected
                while True:
                    yield first
            while True:
                yield from loader
        batches = forever()
    base = None if real else synthetic.stereo_scene(H, b=b, seed=5 + rank, n_view=opt.views)
    z = None
    if model.encoder.__class__.__name__ == "EncoderNotBuilt":
        # torch.channels_last memory: the renderer takes such a level as a view and returns its gradient in the same layout (no copies)
        z = [t.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True) for t in synthetic.feature_maps(b, opt.views, H, seed=1 + rank)]
    optimizer = training.make_adam(params, opt.lr)                  # the reference's Adam and parameter group: what the checkpoint stores
    # the stand-in pyramid (no encoder built) is a per-rank leaf with an optimizer of its own, so that the saved 'optimizer' state matches
    # the reference's param groups
    z_optimizer = training.make_adam(z, opt.lr) if z is not None else None
    if opt.depth and R % 1024:
        raise SystemExit("--depth: the reference's depth-variance term works on 32 x 32 pixel patches (loss_functions.py:112-127): "
                         "--query_sparsity must be a multiple of 1024")
    lpips_w = common.lpips_weights(opt) if opt.lpips else None      # read once per rank; packed on the device at the first step
    patches = opt.depth or opt.lpips
    # a smooth random target image per scene: low-frequency colours of the pixel coordinates
    coef = (torch.rand(b, 3, 4, generator=g) * 2 - 1).to(dev)
    ckpt_dir = os.path.join(opt.logging_root, opt.experiment_name, "checkpoints")
    if rank == 0:
        os.makedirs(ckpt_dir, exist_ok=True)
    # the scene (context images, cameras) goes to the device ONCE; every step only draws new rays there.  (Round 3's loop rebuilt the
    # input dict on the host every step — twelve 65 536-element permutations on the CPU and a 19 MB upload of the context images — and
    # spent 100 ms per step in it; render_train itself queues a step in ~33 ms and the GPU needs ~45 ms: profiles/round4_train_step.md.)
    if not real:
        base = harness.to_device(base, dev, opt.cameras)
    grid = synthetic.pixel_grid(H, H).to(dev)
    gdev = torch.Generator(device=dev).manual_seed(4321 + rank)
    log = val_batches = None
    if rank == 0 and (opt.summaries or opt.val_root):
        from cross_attention_renderer_amd import summaries
        log = summaries.SummaryLog(os.path.join(opt.logging_root, opt.experiment_name, "summaries"))
        if opt.val_root or (not real and opt.val_batch_size > 0):
            val_batches = _validation_batches(opt, model, dev)
    t0, losses, lpips_term, t_warm = time.time(), [], None, None
    for step in range(opt.max_steps):
        if step == min(2, opt.max_steps - 1):                     # steady-state clock: after the first steps' allocations and builds
            torch.cuda.synchronize()
            t_warm = (time.time(), step)
        if real:                                                 # the batch is on the device already: rays, their colours, the mask
            inp, gt = next(batches)
            gt_rgb, mask_scene = gt["rgb"], gt["mask"].to(torch.float32)
        elif patches:                                            # 32 x 32 pixel patches at random corners, row-major inside a patch
            gi = grid.view(H, H, 2)
            corners = torch.randint(0, H - 31, (b, R // 1024, 2), generator=g).tolist()
            uv = torch.stack([torch.cat([gi[y0:y0 + 32, x0:x0 + 32].reshape(1024, 2) for y0, x0 in corners[sc]]) for sc in range(b)])[:, None]
        else:                                                    # R distinct random pixels per scene (query_sparsity), drawn on the device
            uv = torch.stack([grid[torch.randperm(H * H, device=dev, generator=gdev)[:R]] for _ in range(b)])[:, None]   # (b, 1, R, 2)
        if not real:
            inp = {"context": base["context"], "query": dict(base["query"], uv=uv)}
            u = inp["query"]["uv"][:, 0] / (H - 1) * 3.14159
            feats = torch.stack([torch.sin(u[..., 0]), torch.cos(u[..., 1]), torch.sin(u[..., 0] + u[..., 1]), torch.ones_like(u[..., 0])], dim=-1)
            gt_rgb = torch.tanh(torch.einsum("brk,bck->brc", feats, coef))[:, None]                         # (b, 1, R, 3)
        out = model(inp, z=z)                                    # train() mode under autograd = training.render_train (the reference's call, training.py:92)
        loss = img_term = (gt_rgb - out["rgb"]).abs().mean()                                                # loss_functions.image_loss
        if opt.depth:                                            # loss_functions.py:112-127: per-patch depth variance, masked per patch
            d = out["depth_ray"][..., 0].reshape(-1, 1, 32, 32)
            mean = d.mean(dim=-1).mean(dim=-1)[:, None, None]
            dist_ = opt.l2_coeff * torch.pow(d - mean, 2).mean(dim=-1).mean(dim=-1).mean(dim=-1)
            mask = mask_scene if real else torch.ones_like(dist_)  # gt['mask']: every synthetic patch counts
            depth_term = (dist_ * mask).mean()
            loss = loss + depth_term
        if opt.lpips:                                            # loss_functions.py:102-118: LPIPS(gt, pred) per patch, masked per patch
            gt_p, pred_p = gt_rgb.reshape(-1, 32, 32, 3), out["rgb"].reshape(-1, 32, 32, 3)       # channel-last, as car_lpips reads them
            mask = mask_scene if real else torch.ones(gt_p.shape[0], device=dev)   # gt['mask']: every synthetic patch counts
            lpips_term = harness.lpips_loss(gt_p * mask[:, None, None, None], pred_p * mask[:, None, None, None], lpips_w).mean()
            loss = loss + opt.lpips_coeff * lpips_term.to(loss.dtype)
        optimizer.zero_grad()
        if z_optimizer is not None:
            z_optimizer.zero_grad()
        loss.backward()
        if opt.gpus > 1:
            average_gradients(model)                              # the stand-in pyramid, if any, is per rank: not reduced
        torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
        optimizer.step()
        if z_optimizer is not None:
            z_optimizer.step()
        losses.append(loss.detach())                              # no .item() here: that would drain the queue every step
        if log is not None and opt.summaries:                     # training.py:95-116; device values, downloaded at the next flush
            log.add_scalar("img_loss", img_term, step)
            if opt.lpips:
                log.add_scalar("lpips_loss", opt.lpips_coeff * lpips_term.detach(), step)
            if opt.depth:
                log.add_scalar("depth_loss", depth_term, step)
            log.add_scalar("total_at_entropy", summaries.attention_entropy(out["at_wt"].detach(), nan_rows_zero=True), step)
            log.add_scalar("total_train_loss", losses[-1], step)
        if rank == 0 and (step % opt.steps_til_summary == 0 or step == opt.max_steps - 1):
            term = f"  lpips {lpips_term.item():.5f} (x {opt.lpips_coeff:g})" if opt.lpips else ""
            print(f"step {step}: loss {losses[-1].item():.5f}{term}  ({(time.time() - t0) / (step + 1) * 1e3:.1f} ms/step since the start, {b} scenes x {R} rays)", flush=True)
            torch.save({"model": model.state_dict(), "optimizer": optimizer.state_dict()}, os.path.join(ckpt_dir, "model_current.pth"))
            if val_batches is not None:
                _validate(opt, model, next(val_batches), log, step, lpips_w)
            if log is not None:
                log.flush()
        if rank == 0 and step and opt.iters_til_ckpt > 0 and step % opt.iters_til_ckpt == 0:     # training.py:233-235
            epoch = step // len(loader) if real else 0
            torch.save({"model": model.state_dict(), "optimizer": optimizer.state_dict()},
                       os.path.join(ckpt_dir, "model_epoch_%04d_iter_%06d.pth" % (epoch, step)))
    torch.cuda.synchronize()
    if batches is not None:
        batches.close()                                           # stops the reader's threads
    if val_batches is not None:
        val_batches.close()
    if log is not None:
        log.close()
    if rank == 0:
        if t_warm is not None and opt.max_steps - t_warm[1] > 0:
            print(f"steady state: {(time.time() - t_warm[0]) / (opt.max_steps - t_warm[1]) * 1e3:.1f} ms per step over the last {opt.max_steps - t_warm[1]} steps "
                  f"(wall clock, checkpoint writes included)")
        torch.save({"model": model.state_dict(), "optimizer": optimizer.state_dict()}, os.path.join(ckpt_dir, "model_final.pth"))
        print(f"trained {opt.max_steps} steps: loss {losses[0].item():.5f} -> {losses[-1].item():.5f}; wrote {os.path.join(ckpt_dir, 'model_final.pth')}")
    if opt.gpus > 1:
        dist.destroy_process_group()


def _check(opt):
    """Refusals that need no device: they happen before any process opens one."""
    if opt.val_root:
        if not opt.val_pose_root:
            raise SystemExit("--val_root needs --val_pose_root FILE.mat: the validation reader takes its cameras from a .mat pose table")
        if not opt.data_root:
            raise SystemExit("--val_root validates a model trained on --data_root scenes: with synthetic training data --summaries validates on "
                             "a synthetic batch")
    if opt.val_batch_size < (1 if opt.val_root else 0):
        raise SystemExit("--val_batch_size must be at least 1 (0 is allowed with synthetic scenes: no validation pass)")
    if opt.data_root:
        if not opt.pose_root:
            raise SystemExit("--data_root needs --pose_root FILE.mat: the reader takes the cameras from the .mat pose table (scene name -> rows)")
        if opt.depth and not opt.lpips:
            raise SystemExit("--depth on --data_root needs --lpips: the depth-variance term works on 32 x 32 pixel patches "
                             "(loss_functions.py:120-129), and the reference's reader only yields patches under lpips")
    if not opt.lpips:
        return
    if not opt.lpips_weights:
        raise SystemExit("--lpips needs --lpips_weights VGG [LIN]: the loss's forward and backward (harness.lpips_loss) run on the caller's "
                         "LPIPS weight files, and none are shipped")
    if opt.query_sparsity % 1024 and not opt.data_root:           # the reader samples 1024 rays per scene under lpips whatever it says
        raise SystemExit("--lpips: the reference's LPIPS term works on 32 x 32 pixel patches (loss_functions.py:107-109): "
                         "--query_sparsity must be a multiple of 1024")


if __name__ == "__main__":
    opt = _parser().parse_args()
    _check(opt)
    common.spawn(train, opt)
