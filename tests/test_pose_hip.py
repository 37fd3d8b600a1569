"""``-m gpu``: the relative-pose kernels (csrc/car_pose.hip) through the C ABI against the float64 restatement
(tests/pose_reference.py), and ``harness.estimate_pose`` / ``render_unposed_traj.py --matches`` on top of them.

What is compared, and why with these bounds (figures measured on MI355X: profiles/pose_estimate.md):
  * a hypothesis is DECIDED when the restatement's nsol, hyp_best and winning candidate survive relative perturbations of 2^-40 of
    its five points (pose_reference.decided); only decided hypotheses are compared index for index, and at most 5 % may be undecided;
  * residuals of the device's candidates (five epipolar constraints, det E, 2 E E^T E - tr(E E^T) E; E has unit norm, so they are
    relative) against the restatement's worst on the same hypotheses, times the project's margin of 8 and nothing added (measured:
    both sides at 4e-16 or below, the largest ratio of a case 4.7); likewise the noise-free scene's error to the true pose;
  * counts of the device's own candidates against a numpy count of those same matrices: equal;
  * the winner against the restatement's: equal count, hypothesis, candidate and inlier mask; E and (R, t) within 8 x spread + 64 ulp,
    the spread being the largest change of the restatement's own result over 8 perturbed runs.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import pose_reference as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
NS = (5, 6, 64, 1000, 1500)            # the minimum, one more, one LDS chunk, a ragged second chunk, a ragged third
HS = (1, 63, 64, 65, 1024)             # around the solver's 64 lanes and the scorer's 32 hypotheses per workgroup


@pytest.fixture(scope="module")
def dev():
    import torch
    from cross_attention_renderer_amd import _lib
    lib = _lib.load()

    class Dev:
        def up(self, a, dtype):
            return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()            # a copy: the scenes are read-only

        def stream(self):
            return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def stages(self, x0, x1, samples, thresh):
            N, H = len(x0), len(samples)
            d0, d1, ds = self.up(x0, np.float64), self.up(x1, np.float64), self.up(samples, np.int32)
            cand = torch.full((H, 10, 9), float("nan"), dtype=torch.float64, device="cuda")
            nsol = torch.full((H,), -7, dtype=torch.int32, device="cuda")
            counts = torch.full((H, 10), -7, dtype=torch.int32, device="cuda")
            hyp_best = torch.full((H,), -7, dtype=torch.int32, device="cuda")
            E = torch.full((9,), float("nan"), dtype=torch.float64, device="cuda")
            best = torch.full((3,), -7, dtype=torch.int32, device="cuda")
            inl = torch.full((N,), 7, dtype=torch.uint8, device="cuda")
            assert lib.car_essential_solve(d0.data_ptr(), d1.data_ptr(), N, ds.data_ptr(), H, cand.data_ptr(), nsol.data_ptr(), self.stream()) == 0, lib.car_last_error()
            assert lib.car_essential_score(d0.data_ptr(), d1.data_ptr(), N, cand.data_ptr(), nsol.data_ptr(), H, ctypes.c_double(thresh), counts.data_ptr(),
                                           hyp_best.data_ptr(), self.stream()) == 0, lib.car_last_error()
            assert lib.car_essential_select(d0.data_ptr(), d1.data_ptr(), N, cand.data_ptr(), nsol.data_ptr(), counts.data_ptr(), H, ctypes.c_double(thresh),
                                            E.data_ptr(), best.data_ptr(), inl.data_ptr(), self.stream()) == 0, lib.car_last_error()
            torch.cuda.synchronize()
            return dict(cand=cand.cpu().numpy(), nsol=nsol.cpu().numpy(), counts=counts.cpu().numpy(), hyp_best=hyp_best.cpu().numpy(),
                        E=E.cpu().numpy(), best=tuple(int(v) for v in best.cpu().numpy()), inliers=inl.cpu().numpy())

        def ransac(self, x0, x1, samples, thresh, work=None):
            """work: (pointer, bytes) of the caller's own workspace"""
            N, H = len(x0), len(samples)
            d0, d1, ds = self.up(x0, np.float64), self.up(x1, np.float64), self.up(samples, np.int32)
            n = lib.car_essential_workspace_bytes(N, H)
            assert n > 0
            if work is None:
                buf = torch.empty(n, dtype=torch.uint8, device="cuda")
                work = (buf.data_ptr(), n)
            E = torch.full((9,), float("nan"), dtype=torch.float64, device="cuda")
            best = torch.full((3,), -7, dtype=torch.int32, device="cuda")
            inl = torch.full((N,), 7, dtype=torch.uint8, device="cuda")
            assert lib.car_essential_ransac(d0.data_ptr(), d1.data_ptr(), N, ds.data_ptr(), H, ctypes.c_double(thresh), E.data_ptr(), best.data_ptr(),
                                            inl.data_ptr(), work[0], work[1], self.stream()) == 0, lib.car_last_error()
            torch.cuda.synchronize()
            return dict(E=E.cpu().numpy(), best=tuple(int(v) for v in best.cpu().numpy()), inliers=inl.cpu().numpy())
    return Dev()


_scenes = {}


def scene_of(N):
    """One noisy scene per N (half a pixel of noise, 40 % outliers from 64 matches up), normalised; computed once and never changed."""
    if N not in _scenes:
        k0, k1, R, t, _ = P.scene(N, 40 + N, noise=0.5, outliers=0.4 if N >= 64 else 0.0)
        x0, x1, nt = P.normalise(k0, k1, P.K, P.K, 1.0)
        for a in (k0, k1, x0, x1):
            a.setflags(write=False)
        _scenes[N] = (k0, k1, x0, x1, nt, R, t)
    return _scenes[N]


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("N", NS)
def test_stages_against_the_restatement(dev, N, H):
    _, _, x0, x1, nt, _, _ = scene_of(N)
    S = P.sample_table(N, H, seed=N)
    ref = P.ransac(x0, x1, S, nt)
    dec = P.decided(x0, x1, S, nt, base=ref)
    got = dev.stages(x0, x1, S, nt)
    print(f"N={N} H={H}: undecided {(~dec).sum()} of {H}; nsol histogram {np.bincount(got['nsol'], minlength=11).tolist()}")
    assert (~dec).mean() <= 0.05
    assert ((got["nsol"] >= 0) & (got["nsol"] <= 10)).all()
    assert (got["cand"][np.arange(10)[None, :] >= got["nsol"][:, None]] == 0).all()                  # unused slots are zero
    assert (got["nsol"] == ref["nsol"])[dec].all()

    # candidates: unit norm, and the three constraints against the restatement's own worst residual on the same hypotheses
    used = np.arange(10)[None, :] < got["nsol"][:, None]
    assert np.abs(np.linalg.norm(got["cand"], axis=2)[used] - 1.0).max(initial=0.0) <= 8 * EPS
    r_dev, r_ref = P.residuals(got["cand"], got["nsol"], x0, x1, S)[dec], P.residuals(ref["cand"], ref["nsol"], x0, x1, S)[dec]
    for k, name in enumerate(("epipolar", "det", "trace")):
        worst_dev, worst_ref = r_dev[..., k].max(initial=0.0), r_ref[..., k].max(initial=0.0)
        print(f"  {name:8s} worst residual: device {worst_dev:.3e}  restatement {worst_ref:.3e}")
        assert worst_dev <= 8 * worst_ref, name

    # counts of the device's own candidates: a numpy count of those same matrices
    counts, hyp_best = P.score(got["cand"], got["nsol"], x0, x1, nt)
    assert np.array_equal(got["counts"], counts) and np.array_equal(got["hyp_best"], hyp_best)
    assert np.array_equal(got["hyp_best"][dec], ref["hyp_best"][dec])

    # the winner: the tie rule on the device's own arrays, the one-call entry, and the restatement's winner
    E, best, inl = P.select(got["cand"], got["nsol"], got["counts"], x0, x1, nt)
    assert got["best"] == best and np.array_equal(got["E"], E) and np.array_equal(got["inliers"], inl)
    one = dev.ransac(x0, x1, S, nt)
    assert one["best"] == got["best"] and one["E"].tobytes() == got["E"].tobytes() and np.array_equal(one["inliers"], got["inliers"])
    cnt, h, c = ref["best"]
    err = P.sampson(ref["E"], x0, x1)
    assert dec[h] and np.abs(err - nt * nt).min() > 1e-9 * nt * nt, "the scene is no fair test: its winner is undecided or a match sits on the threshold"
    spread = P.winner_spread(x0, x1, S[h], c)
    diff = min(np.abs(one["E"] - ref["E"]).max(), np.abs(one["E"] + ref["E"]).max())
    print(f"  winner {one['best']} (restatement {ref['best']}); |E - E_ref| {diff:.3e}, spread {spread:.3e}")
    assert one["best"] == ref["best"] and np.array_equal(one["inliers"], ref["inliers"])
    assert diff <= 8 * spread + 64 * EPS


@pytest.mark.parametrize("N,H", [(64, 65), (1000, 1024)])
def test_estimate_pose_against_the_restatement(dev, N, H):
    from cross_attention_renderer_amd import harness
    k0, k1, x0, x1, nt, R, t = scene_of(N)
    assert np.array_equal(harness.pose_sample_table(N, H, 3), P.sample_table(N, H, 3))
    got = harness.estimate_pose(k0, k1, P.K, P.K, 1.0, hypotheses=H, seed=3)
    ref = P.estimate(k0, k1, P.K, P.K, 1.0, hypotheses=H, seed=3)
    assert got is not None and ref is not None
    _, h, c = ref[3]["best"]
    spread = P.winner_spread(x0, x1, P.sample_table(N, H, 3)[h], c, fn=lambda E, a, b: P.pose_of(E, a, b, nt))
    dR, dt = np.abs(got[0] - ref[0]).max(), np.abs(got[1] - ref[1]).max()
    print(f"N={N} H={H}: |R - R_ref| {dR:.3e} |t - t_ref| {dt:.3e} spread {spread:.3e}; inliers {got[2].sum()}; "
          f"to the true pose: R {np.degrees(P.rot_angle(got[0], R)):.3f} deg, t {np.degrees(P.dir_angle(got[1], t)):.3f} deg")
    assert max(dR, dt) <= 8 * spread + 64 * EPS
    assert np.array_equal(got[2], ref[2]) and got[2].dtype == bool
    assert abs(np.linalg.norm(got[1]) - 1.0) <= 8 * EPS and abs(np.linalg.det(got[0]) - 1.0) <= 64 * EPS
    assert harness.estimate_pose(k0[:4], k1[:4], P.K, P.K, 1.0) is None


def test_noise_free_scene_recovers_the_true_pose(dev):
    from cross_attention_renderer_amd import harness
    k0, k1, R, t, _ = P.scene(200, 11)
    got = harness.estimate_pose(k0, k1, P.K, P.K, 1.0, hypotheses=64, seed=0)
    ref = P.estimate(k0, k1, P.K, P.K, 1.0, hypotheses=64, seed=0)
    e_dev = max(np.abs(got[0] - R).max(), np.abs(got[1] - t).max())          # entrywise: arccos near 1 resolves angles only to sqrt(eps)
    e_ref = max(np.abs(ref[0] - R).max(), np.abs(ref[1] - t).max())
    print(f"noise-free: error to the true pose, device {e_dev:.3e}, restatement {e_ref:.3e}")
    assert got[2].all() and e_dev <= 8 * e_ref


def test_hostile_tables_and_points(dev):
    N, H = 64, 65
    _, _, x0, x1, nt, _, _ = scene_of(N)
    S = P.sample_table(N, H, seed=5)
    bad = {3: [0, 1, 2, 3, N], 17: [4, 4, 5, 6, 7], 40: [-1, 1, 2, 3, 4], 63: [2 ** 31 - 1, 1, 2, 3, 4], 64: [9, 8, 7, 6, 9], 0: [-2 ** 31, 5, 6, 7, 8]}
    T = S.copy()
    for row, v in bad.items():
        T[row] = v
    got = dev.stages(x0, x1, T, nt)
    clean = dev.stages(x0, x1, S, nt)
    keep = np.array([h for h in range(H) if h not in bad])
    assert (got["nsol"][sorted(bad)] == 0).all() and np.array_equal(got["nsol"][keep], clean["nsol"][keep])
    assert got["cand"][keep].tobytes() == clean["cand"][keep].tobytes() and (got["counts"][sorted(bad)] == 0).all()
    only = dev.ransac(x0, x1, S[keep], nt)
    mixed = dev.ransac(x0, x1, T, nt)
    assert mixed["E"].tobytes() == only["E"].tobytes() and np.array_equal(mixed["inliers"], only["inliers"])
    assert mixed["best"] == (only["best"][0], int(keep[only["best"][1]]), only["best"][2])

    # a non-finite sample point refuses its hypotheses; a non-finite match is never an inlier
    for poison in (np.nan, np.inf, -np.inf):
        y0, y1 = x0.copy(), x1.copy()
        y0[7, 1] = poison
        y1[21, 0] = poison
        got = dev.stages(y0, y1, S, nt)
        hit = ((S == 7) | (S == 21)).any(axis=1)
        assert hit.any() and (got["nsol"][hit] == 0).all() and (got["nsol"][~hit] == clean["nsol"][~hit]).all()
        counts, _ = P.score(got["cand"], got["nsol"], y0, y1, nt)
        assert np.array_equal(got["counts"], counts)
        assert got["inliers"][7] == 0 and got["inliers"][21] == 0 and got["best"][0] > 0


def test_degenerate_scenes_terminate(dev):
    from cross_attention_renderer_amd import harness
    g = np.random.default_rng(0)
    s = g.uniform(-0.4, 0.4, size=64)
    line0 = np.stack([s, 0.5 * s + 0.1], axis=1)
    line1 = np.stack([s, 0.5 * s + 0.1], axis=1) + 0.05
    same = np.tile([[0.1, -0.2]], (64, 1))
    S = P.sample_table(64, 65, 0)
    for a, b in ((line0, line1), (same, same), (np.zeros((64, 2)), np.zeros((64, 2)))):
        got = dev.stages(a, b, S, 1.0 / 225.0)                              # returns: every loop of the solver is bounded
        assert ((got["nsol"] >= 0) & (got["nsol"] <= 10)).all()
        out = harness.estimate_pose(a * 225 + 128, b * 225 + 128, P.K, P.K, 1.0, hypotheses=65)
        assert out is None or (np.isfinite(out[0]).all() and np.isfinite(out[1]).all())
    got = dev.stages(same, same, S, 1.0 / 225.0)
    assert (got["nsol"] == 0).all() and got["best"] == (0, -1, -1) and not got["inliers"].any() and not got["E"].any()
    assert harness.estimate_pose(same * 225 + 128, same * 225 + 128, P.K, P.K, 1.0, hypotheses=65) is None


def test_two_runs_give_identical_bytes(dev):
    _, _, x0, x1, nt, _, _ = scene_of(1000)
    S = P.sample_table(1000, 1024, seed=9)
    a, b = dev.stages(x0, x1, S, nt), dev.stages(x0, x1, S, nt)
    for k in ("cand", "nsol", "counts", "hyp_best", "E", "inliers"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["best"] == b["best"]
    c, d = dev.ransac(x0, x1, S, nt), dev.ransac(x0, x1, S, nt)
    assert c["E"].tobytes() == d["E"].tobytes() == a["E"].tobytes() and c["best"] == d["best"] and np.array_equal(c["inliers"], d["inliers"])


def test_ransac_fits_its_workspace_exactly(dev):
    """N = 6 matches, H = 3 hypotheses: the three int pieces of the workspace end off a 16-byte boundary.  A workspace of exactly
    car_essential_workspace_bytes, NaN all around it, then one twice as large: nothing is written outside either, the results are the
    same bytes, and they are the stage entries' on arrays of their own."""
    import abi_harness as A
    from cross_attention_renderer_amd import _lib
    N, H = 6, 3
    _, _, x0, x1, nt, _, _ = scene_of(N)
    S = P.sample_table(N, H, seed=N)

    def run(work, work_bytes):
        one = dev.ransac(x0, x1, S, nt, work=(work.ptr, work_bytes))
        return one["E"], np.array(one["best"], dtype=np.int32), one["inliers"]

    E, best, inl = A.exact_then_twice(_lib.load().car_essential_workspace_bytes(N, H), run, "car_essential_ransac")
    got = dev.stages(x0, x1, S, nt)
    assert tuple(best) == got["best"] and E.tobytes() == got["E"].tobytes() and np.array_equal(inl, got["inliers"])


def test_ties_go_to_the_lower_index(dev):
    _, _, x0, x1, nt, _, _ = scene_of(64)
    S = P.sample_table(64, 65, seed=2)
    first = dev.ransac(x0, x1, S, nt)
    _, w, c = first["best"]
    assert w > 0
    front = dev.ransac(x0, x1, np.concatenate([S[w:w + 1], S, S[w:w + 1]]), nt)          # the winner's row again, before and after
    assert front["best"] == (first["best"][0], 0, c) and front["E"].tobytes() == first["E"].tobytes()
    back = dev.ransac(x0, x1, np.concatenate([S, S[w:w + 1]]), nt)                       # only after: the first copy keeps winning
    assert back["best"] == first["best"] and back["E"].tobytes() == first["E"].tobytes()


def test_script_renders_from_a_matches_file(dev, tmp_path):
    from cross_attention_renderer_amd import harness, trajectory
    k0, k1, R, t, _ = P.scene(300, 21, noise=0.5, outliers=0.3)
    g = np.random.default_rng(1)
    kp0 = np.concatenate([k0, g.uniform(0, 256, size=(40, 2))]).astype(np.float32)          # 40 keypoints without a partner
    order = g.permutation(300)
    kp1 = np.concatenate([k1[order], g.uniform(0, 256, size=(25, 2))]).astype(np.float32)
    matches = np.concatenate([np.argsort(order), -np.ones(40, dtype=np.int64)])
    path = tmp_path / "pair_matches.npz"
    np.savez(path, keypoints0=kp0, keypoints1=kp1, matches=matches, match_confidence=np.ones(340, dtype=np.float32))
    m0, m1, conf = trajectory.read_matches(str(path))
    assert np.array_equal(m0, k0.astype(np.float32)) and np.array_equal(m1, k1.astype(np.float32)) and conf.shape == (300,)
    cmd = [sys.executable, os.path.join(ROOT, "experiment_scripts", "render_unposed_traj.py"), "--experiment_name", "t", "--views", "2", "--synthetic",
           "--matches", str(path), "--pose_hypotheses", "512", "--n_frames", "2", "--out_dir", str(tmp_path), "--logging_root", str(tmp_path)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert (tmp_path / "frame_0001.png").exists() and "rendered 2 frames" in out.stdout and "inliers" in out.stdout
    K = trajectory.UNPOSED_K[:3, :3]
    want = harness.estimate_pose(m0, m1, K, K, 1.0, hypotheses=512)
    used = np.load(tmp_path / "pose.npz")
    assert np.array_equal(used["R"], want[0]) and np.array_equal(used["t"], want[1]) and np.array_equal(used["inliers"], want[2])
    assert f"{int(want[2].sum())} inliers" in out.stdout
    assert np.degrees(P.rot_angle(want[0], R)) < 2.0 and np.degrees(P.dir_angle(want[1], t)) < 4.0, "the estimate is nowhere near the scene's pose"
    bad = subprocess.run(cmd[:2] + ["--experiment_name", "t", "--im1", "a.npy", "--im2", "b.npy"], capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "exactly one of --matches" in bad.stderr
