"""Novel views from two images of unknown pose (mirrors reference experiment_scripts/render_unposed_traj.py).

    python experiment_scripts/render_unposed_traj.py --experiment_name demo --checkpoint_path model.pth --im1 a.png --im2 b.png --matches m.npz
    python experiment_scripts/render_unposed_traj.py --experiment_name demo --checkpoint_path model.pth --im1 a.png --im2 b.png --pose rt.npz
    python experiment_scripts/render_unposed_traj.py --experiment_name demo --checkpoint_path model.pth --im1 a.png --im2 b.png \
        --matcher_weights superpoint_v1.pth superglue_indoor.pth

The reference gets the relative pose of the second image in two steps (dataset/load_video_superglue.py:419-479): SuperPoint + SuperGlue
match keypoints of the two 256 x 256 crops, then ``estimate_pose`` (:114-138) runs ``cv2.findEssentialMat`` (RANSAC) and
``cv2.recoverPose`` on the matches.  Both steps are here.  ``--matcher_weights SUPERPOINT.pth SUPERGLUE.pth`` runs the first on the
device (``matching.match_pair``) with the caller's copies of the published weight files — none are shipped — on the
grey images 0.2125 R + 0.7154 G + 0.0721 B (skimage's rgb2gray) of the two 256 x 256 crops, with the reference's configuration (:421-432);
``--save_matches OUT.npz`` writes what it found in the layout below.  For the second step alone, ``--matches`` takes the .npz that SuperGlue's published ``match_pairs.py`` writes for the pair (``keypoints0``, ``keypoints1``,
``matches``, ``match_confidence``; ``trajectory.read_matches``) and ``harness.estimate_pose`` estimates (R, t) from it on the device,
with K = ``trajectory.UNPOSED_K`` and a threshold of 1 pixel as the reference sets them, and prints the inlier count.  The keypoints are
pixels of the 256 x 256 CROPS: run the matcher on the centre-cropped, resized images, as the reference does, not on the photographs.
The estimator is not cv2's: a fixed budget of ``--pose_hypotheses`` five-point samples, all scored, replaces cv2's early stop, and
neither it nor the host's recoverPose is pinned against cv2.  ``--pose`` instead takes (R, t) —
``recoverPose``'s convention, x_2 = R x_1 + t — from an .npz with ``R`` (3, 3) and ``t`` (3,) estimated elsewhere.  With --im1 / --im2
exactly one of the three is required; no two of them go together.

Everything after that is the reference's path: the two images centre-cropped to squares and scaled to [-1, 1], first camera =
world frame, second at inv([R | t]) with its position divided by 1.2, fixed RealEstate10K intrinsics, 76 query poses on a helix
between the two (``trajectory.unposed_pair_input``, pinned in tests/test_trajectory.py), ``get_z`` once, one chunked forward per
pose, frames written as PNG.  Images must already be 256 pixels high (the reference resizes with skimage, not installed here).
--synthetic renders the same trajectory over the seeded synthetic pair and feature pyramid; with --matches or --matcher_weights (which
then matches the synthetic pair's two images) its pose is the estimator's too, and the pose used is written to ``pose.npz`` beside the frames."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import common  # noqa: E402


def _read_image(path):
    import numpy as np
    if path.endswith(".npy"):
        im = np.load(path)
    else:
        from PIL import Image
        im = np.asarray(Image.open(path).convert("RGB"))
    im = im.astype(np.float64) / 255.0 if im.dtype == np.uint8 else im.astype(np.float64)
    from cross_attention_renderer_amd.trajectory import center_crop_square
    im = center_crop_square(im)
    if im.shape[:2] != (256, 256):
        raise SystemExit(f"{path}: {im.shape[0]}x{im.shape[1]} after the centre crop; the renderer works at 256x256 — resize the image first")
    return im


def pose_sources(opt):
    """The ways to the relative pose that the arguments name: --matches, --pose, --matcher_weights."""
    return [n for n in ("matches", "pose", "matcher_weights") if getattr(opt, n)]


def check_pose_sources(opt):
    """No two sources together; with --im1 / --im2 (and no --synthetic) exactly one.  The wording for `none` and for --matches with
    --pose is the one the script always had."""
    given = pose_sources(opt)
    if opt.save_matches and not opt.matcher_weights:
        raise SystemExit("--save_matches writes what --matcher_weights finds: it needs --matcher_weights")
    if opt.im1 and opt.im2 and not opt.synthetic and not opt.matcher_weights and bool(opt.pose) == bool(opt.matches):
        raise SystemExit("--im1 / --im2 need exactly one of --matches (SuperGlue's .npz for the pair) and --pose (an .npz with R, t)")
    if len(given) > 1:
        raise SystemExit(f"--{given[0]} and --{given[1]} both name the relative pose: give exactly one of --matches, --pose and --matcher_weights")


def gray(im):
    """skimage.color.rgb2gray's weights, as the reference applies them to the [0, 1] crops (load_video_superglue.py:446-447)."""
    return 0.2125 * im[..., 0] + 0.7154 * im[..., 1] + 0.0721 * im[..., 2]


def match_images(opt, im0, im1, dev, rank):
    """--matcher_weights: SuperPoint + SuperGlue on the two [0, 1] crops; the matched keypoints, and --save_matches' file."""
    import numpy as np
    import torch
    from cross_attention_renderer_amd import matching
    weights = matching.load_matcher_weights(*opt.matcher_weights)
    g0, g1 = (torch.from_numpy(np.ascontiguousarray(gray(im))).to(dev, torch.float32) for im in (im0, im1))
    pred = {k: v.cpu().numpy() for k, v in matching.match_pair(g0, g1, weights).items()}
    m = pred["matches0"]
    if opt.save_matches and rank == 0:
        np.savez(opt.save_matches, keypoints0=pred["keypoints0"], keypoints1=pred["keypoints1"], matches=m, match_confidence=pred["matching_scores0"])
    valid = m > -1
    if rank == 0:
        print(f"matched {int(valid.sum())} of {len(m)} and {len(pred['keypoints1'])} keypoints")
    return pred["keypoints0"][valid], pred["keypoints1"][m[valid]]


def render(rank, opt):
    import numpy as np
    import torch
    from cross_attention_renderer_amd import harness, synthetic, trajectory
    dev = common.init_rank(rank, opt)
    H = 256
    opt.img_sidelength = H
    uv = synthetic.pixel_grid(H, H)
    check_pose_sources(opt)
    real = not (opt.synthetic or not (opt.im1 and opt.im2 and pose_sources(opt)))
    images = None
    if opt.matcher_weights:
        g = np.random.default_rng(0)
        images = (_read_image(opt.im1), _read_image(opt.im2)) if real else (g.random((H, H, 3)), g.random((H, H, 3)))
    estimated = None
    if opt.matches or opt.matcher_weights:
        if opt.matches:
            mkpts0, mkpts1, _ = trajectory.read_matches(opt.matches)
        else:
            mkpts0, mkpts1 = match_images(opt, *images, dev, rank)
        K = trajectory.UNPOSED_K[:3, :3]
        estimated = harness.estimate_pose(mkpts0, mkpts1, K, K, 1.0, hypotheses=opt.pose_hypotheses, device=dev)
        if estimated is None:
            raise SystemExit(f"{opt.matches or 'the matcher'}: no relative pose from its {len(mkpts0)} matches (at least five good ones are needed)")
        if rank == 0:
            print(f"pose from {len(mkpts0)} matches, {opt.pose_hypotheses} hypotheses: {int(estimated[2].sum())} inliers")
    if not real:
        model = common.build_model(opt, dev)
        g = np.random.default_rng(0)
        yaw = np.deg2rad(-12.0)
        R = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]]).T
        t = -R @ np.array([0.6, 0.03, 0.05])
        if estimated is not None:
            R, t = estimated[:2]
        inp = trajectory.unposed_pair_input(g.random((H, H, 3)), g.random((H, H, 3)), R, t, uv)
        z = [t.to(dev) for t in synthetic.feature_maps(1, 2, H, seed=1)]
        inp = harness.to_device(inp, dev, opt.cameras)
    else:
        model = common.build_model(opt, dev, with_encoder=True)
        if estimated is not None:
            R, t = estimated[:2]
        else:
            rt = np.load(opt.pose)
            R, t = rt["R"], rt["t"]
        im1, im2 = images or (_read_image(opt.im1), _read_image(opt.im2))
        inp = harness.to_device(trajectory.unposed_pair_input(im1, im2, R, t, uv), dev, opt.cameras)
        with torch.no_grad():
            z = model.get_z(inp)
    out_dir = opt.out_dir or os.path.join(opt.logging_root, opt.experiment_name, "unposed")
    if rank == 0:
        os.makedirs(out_dir, exist_ok=True)
        if estimated is not None:
            np.savez(os.path.join(out_dir, "pose.npz"), R=estimated[0], t=estimated[1], inliers=estimated[2])
    nq = inp["query"]["cam2world"].shape[1] if not opt.n_frames else min(opt.n_frames, inp["query"]["cam2world"].shape[1])
    for i in range(nq):
        frame = {"context": inp["context"], "query": {"cam2world": inp["query"]["cam2world"][:, i:i + 1], "intrinsics": inp["query"]["intrinsics"][:, i:i + 1],
                                                       "uv": inp["query"]["uv"][:, i:i + 1].contiguous()}}
        tile = harness.render_frame(model, frame, z, rank=rank, world=opt.gpus)          # 8192-ray chunks (render_unposed_traj.py:73)
        if rank == 0:
            harness.write_png(os.path.join(out_dir, f"frame_{i:04d}.png"), tile[0, :, :3].reshape(H, H, 3))
    torch.cuda.synchronize()
    if rank == 0:
        print(f"rendered {nq} frames -> {out_dir}")


if __name__ == "__main__":
    p = common.add_precision(common.parser(__doc__))
    p.add_argument("--im1", type=str, default=None)
    p.add_argument("--im2", type=str, default=None)
    p.add_argument("--pose", type=str, default=None, help=".npz with R (3,3), t (3,) of the second camera relative to the first")
    p.add_argument("--matches", type=str, default=None,
                   help=".npz of SuperGlue's match_pairs.py for the pair (keypoints0, keypoints1, matches, match_confidence; pixels of the "
                        "256x256 crops): the relative pose is estimated from it on the device")
    p.add_argument("--matcher_weights", type=str, nargs=2, default=None, metavar=("SUPERPOINT.pth", "SUPERGLUE.pth"),
                   help="the published SuperPoint and SuperGlue state dicts: the two crops are matched on the device and the pose is estimated from the matches")
    p.add_argument("--save_matches", type=str, default=None, help=".npz to write --matcher_weights' keypoints and matches to, in the layout --matches reads")
    p.add_argument("--pose_hypotheses", type=int, default=8192, help="five-point hypotheses the pose estimator solves and scores (--matches, --matcher_weights)")
    opt = p.parse_args()
    common.spawn(render, opt)
