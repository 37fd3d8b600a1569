"""CPU: the float64 restatement of the relative-pose estimator (tests/pose_reference.py) against ground truth, ``trajectory.read_matches``,
and the refusals of the C entries (include/car_hip.h: car_essential_*).  The GPU tests (tests/test_pose_hip.py) then hold the kernels to
this restatement.

Bounds of the noisy scenes: measured with this file's budget (512 matches, 4096 hypotheses, half a pixel of noise, seeds 100-107 of
pose_reference.scene; profiles/pose_estimate.md), worst of the 8 seeds, times 2 because seeds vary:
    inliers   winner's shortfall to the true pose's count   R error   t direction error
    60 %      3.4 %                                         0.90 deg  1.41 deg
    40 %      9.0 %                                         1.74 deg  1.61 deg
    30 %      19.0 %                                        2.92 deg  3.92 deg
"""
import ctypes

import numpy as np
import pytest

import pose_reference as P

EPS = np.finfo(np.float64).eps
N_NOISY, H_NOISY, NOISE = 512, 4096, 0.5
BOUNDS = {0.6: (2 * 0.034, 2 * 0.90, 2 * 1.41), 0.4: (2 * 0.090, 2 * 1.74, 2 * 1.61), 0.3: (2 * 0.190, 2 * 2.92, 2 * 3.92)}

_noisy = {}


def noisy(share):
    """The estimate of one noisy scene per inlier share, computed once and shared."""
    if share not in _noisy:
        k0, k1, R, t, _ = P.scene(N_NOISY, 100, NOISE, 1.0 - share)
        x0, x1, nt = P.normalise(k0, k1, P.K, P.K, 1.0)
        S = P.sample_table(N_NOISY, H_NOISY, 0)
        _noisy[share] = (x0, x1, nt, R, t, S, P.estimate(k0, k1, P.K, P.K, 1.0, samples=S))
    return _noisy[share]


def test_sample_table():
    from cross_attention_renderer_amd import harness
    for n, h in ((5, 200), (6, 200), (1000, 4096)):
        S = P.sample_table(n, h, 7)
        assert S.dtype == np.int32 and S.shape == (h, 5) and S.min() >= 0 and S.max() < n
        assert (np.diff(np.sort(S, axis=1), axis=1) > 0).all()
        assert np.array_equal(S, harness.pose_sample_table(n, h, 7))
    assert not np.array_equal(P.sample_table(1000, 64, 0), P.sample_table(1000, 64, 1))


@pytest.mark.parametrize("seed", [1, 2])
def test_noise_free_true_essential_is_a_candidate_and_the_pose_comes_back(seed):
    k0, k1, R, t, _ = P.scene(64, seed)
    x0, x1, nt = P.normalise(k0, k1, P.K, P.K, 1.0)
    S = P.sample_table(64, 512, seed)
    base = P.ransac(x0, x1, S, nt)
    dec = P.decided(x0, x1, S, nt, base=base)
    assert (~dec).mean() <= 0.05 and (base["nsol"][dec] > 0).all()
    Et = P.true_E(R, t)
    d = np.minimum(np.abs(base["cand"] - Et).max(axis=2), np.abs(base["cand"] + Et).max(axis=2))
    d = np.where(np.arange(10)[None, :] < base["nsol"][:, None], d, np.inf)
    near, dist = d.argmin(axis=1), d.min(axis=1)
    # the yardstick: how far that same candidate moves when the five points move by 2^-40 (4096 times their rounding)
    moved = np.zeros(len(S))
    for k in range(2):
        cand, nsol = P.solve(*P.perturbed(x0, x1, k), S)
        moved = np.maximum(moved, np.abs(cand - base["cand"])[np.arange(len(S)), near].max(axis=1))
    print(f"seed {seed}: undecided {(~dec).sum()}, worst distance to the true E {dist[dec].max():.3e}, its yardstick {moved[dec][dist[dec].argmax()]:.3e}")
    assert (dist[dec] <= 8 * moved[dec] + 64 * EPS).all()
    assert (base["hyp_best"][dec] == 64).all() and base["best"][0] == 64 and base["inliers"].all()

    out = P.estimate(k0, k1, P.K, P.K, 1.0, samples=S)
    _, h, c = out[3]["best"]
    spread = P.winner_spread(x0, x1, S[h], c, fn=lambda E, a, b: P.pose_of(E, a, b, nt))
    err = max(np.abs(out[0] - R).max(), np.abs(out[1] - t).max())
    print(f"seed {seed}: |R - R_true|, |t - t_true| <= {err:.3e}; spread {spread:.3e}")
    assert err <= 8 * spread + 64 * EPS and out[2].all()
    assert abs(np.linalg.det(out[0]) - 1) <= 64 * EPS and abs(np.linalg.norm(out[1]) - 1) <= 8 * EPS


@pytest.mark.parametrize("share", [0.6, 0.4, 0.3])
def test_noisy_scenes_reach_the_true_poses_support(share):
    x0, x1, nt, R, t, S, out = noisy(share)
    assert out is not None
    true_count = int((P.sampson(P.true_E(R, t), x0, x1) < nt * nt).sum())
    count, h, c = out[3]["best"]
    e_R, e_t = np.degrees(P.rot_angle(out[0], R)), np.degrees(P.dir_angle(out[1], t))
    short, b_R, b_t = BOUNDS[share]
    print(f"{share:.0%} inliers: true pose {true_count}, winner {count} (shortfall {(true_count - count) / true_count:.3f}); R {e_R:.3f} deg, t {e_t:.3f} deg")
    assert count >= true_count * (1.0 - short) and e_R <= b_R and e_t <= b_t
    # conditions of a fair scene: no match on the threshold under the winner; the winner decided; at most 5 % undecided.  The last is
    # checked on the first 512 rows, a SAMPLE: the rows of a table are independent draws, so a prefix is an unbiased sample of it (a
    # share of 5 % would show as 26 +- 5 rows; 0 or 1 are measured), and deciding all 4096 rows would triple this test's time.  The
    # GPU tests decide every row of their tables.
    assert np.abs(P.sampson(out[3]["E"], x0, x1) - nt * nt).min() > 1e-9 * nt * nt
    rows = np.unique(np.concatenate([np.arange(512), [h]]))
    dec = P.decided(x0, x1, S[rows], nt)
    assert (~dec).mean() <= 0.05 and dec[np.searchsorted(rows, h)]
    assert out[2].sum() <= count and out[2].sum() >= 0.9 * count                            # cheirality drops few of the winner's inliers


def test_a_longer_table_never_finds_fewer_inliers():
    x0, x1, nt, _, _, S, out = noisy(0.3)
    r = out[3]
    last = 0
    for h in (1, 8, 64, 300, 1000, 4096):
        _, best, _ = P.select(r["cand"][:h], r["nsol"][:h], r["counts"][:h], x0, x1, nt)
        assert best[0] >= last and best[0] == r["hyp_best"][:h].max()
        last = best[0]
    assert last == r["best"][0]


def test_recover_pose_picks_the_combination_in_front_of_both_cameras():
    from cross_attention_renderer_amd import harness
    k0, k1, R, t, _ = P.scene(40, 5)
    x0, x1, _ = P.normalise(k0, k1, P.K, P.K, 1.0)
    for sign in (1.0, -1.0):                                                                  # E is known up to sign only
        for fn in (P.recover_pose, harness.recover_pose):
            n, Rr, tr, mask = fn(sign * P.true_E(R, t), x0, x1, np.ones(40, dtype=np.uint8))
            assert n == 40 and mask.all() and np.abs(Rr - R).max() < 1e-12 and np.abs(tr - t).max() < 1e-12
    n, _, _, mask = harness.recover_pose(P.true_E(R, t), x0, x1, np.arange(40) < 10)
    assert n == 10 and mask.sum() == 10 and not mask[10:].any()


def test_read_matches(tmp_path):
    from cross_attention_renderer_amd import trajectory
    g = np.random.default_rng(0)
    kp0, kp1 = g.uniform(0, 256, size=(7, 2)).astype(np.float32), g.uniform(0, 256, size=(5, 2)).astype(np.float32)
    matches, conf = np.array([3, -1, 0, -1, 4, 1, -1]), np.linspace(0.2, 0.9, 7).astype(np.float32)
    path = str(tmp_path / "a_b_matches.npz")
    np.savez(path, keypoints0=kp0, keypoints1=kp1, matches=matches, match_confidence=conf)
    m0, m1, mc = trajectory.read_matches(path)
    assert np.array_equal(m0, kp0[[0, 2, 4, 5]]) and np.array_equal(m1, kp1[[3, 0, 4, 1]]) and np.array_equal(mc, conf[[0, 2, 4, 5]])
    np.savez(path, keypoints0=kp0, keypoints1=kp1, matches=matches)
    with pytest.raises(ValueError, match="match_confidence"):
        trajectory.read_matches(path)


def test_estimate_pose_needs_five_matches_and_has_no_cpu_fallback():
    import torch
    from cross_attention_renderer_amd import harness
    k = np.zeros((4, 2))
    assert harness.estimate_pose(k, k, P.K, P.K, 1.0) is None
    with pytest.raises(ValueError):
        harness.estimate_pose(np.zeros((6, 3)), np.zeros((6, 3)), P.K, P.K, 1.0)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            harness.estimate_pose(np.zeros((6, 2)), np.zeros((6, 2)), P.K, P.K, 1.0)


def test_c_entries_refuse_with_codes():
    """Sizes without a GPU; every refusal is a code and a message, never an abort (nothing is launched on a refusal)."""
    import __graft_entry__ as ge
    ge.build()
    from cross_attention_renderer_amd import _lib
    lib = _lib.load()
    up16 = lambda n: (n + 15) // 16 * 16
    for n, h in ((5, 1), (1000, 8192), (1500, 65)):
        assert lib.car_essential_workspace_bytes(n, h) == up16(h * 720) + up16(4 * h) + up16(40 * h) + up16(4 * h)
    for n, h in ((4, 8), (0, 8), (-1, 8), (5, 0), (5, -3), (2 ** 24 + 1, 8), (5, 2 ** 24 + 1)):
        assert lib.car_essential_workspace_bytes(n, h) == 0 and b"car_essential_workspace_bytes" in lib.car_last_error()
    buf = (ctypes.c_double * 4096)()                                                          # a host array: never dereferenced by a refusal
    p = ctypes.cast(buf, ctypes.c_void_p)
    th = ctypes.c_double(0.004)
    assert lib.car_essential_solve(None, p, 8, p, 4, p, p, None) == -1 and b"null pointer" in lib.car_last_error()
    assert lib.car_essential_solve(p, p, 4, p, 4, p, p, None) == -1 and b"N = 4" in lib.car_last_error()
    assert lib.car_essential_solve(p, p, 8, p, 0, p, p, None) == -1 and b"H = 0" in lib.car_last_error()
    assert lib.car_essential_score(p, p, 8, p, None, 4, th, p, p, None) == -1 and b"null pointer" in lib.car_last_error()
    assert lib.car_essential_score(p, p, 8, p, p, 4, ctypes.c_double(0.0), p, p, None) == -1 and b"thresh" in lib.car_last_error()
    assert lib.car_essential_score(p, p, 8, p, p, 4, ctypes.c_double(float("nan")), p, p, None) == -1
    assert lib.car_essential_select(p, p, 8, p, p, p, 4, th, p, None, p, None) == -1 and b"null pointer" in lib.car_last_error()
    assert lib.car_essential_select(p, p, 8, p, p, p, 4, ctypes.c_double(-1.0), p, p, p, None) == -1 and b"thresh" in lib.car_last_error()
    need = lib.car_essential_workspace_bytes(8, 4)
    assert lib.car_essential_ransac(p, p, 8, p, 4, th, p, p, p, None, need, None) == -1 and b"null pointer" in lib.car_last_error()
    assert lib.car_essential_ransac(p, p, 4, p, 4, th, p, p, p, p, need, None) == -1 and b"N = 4" in lib.car_last_error()
    assert lib.car_essential_ransac(p, p, 8, p, -1, th, p, p, p, p, need, None) == -1 and b"H = -1" in lib.car_last_error()
    assert lib.car_essential_ransac(p, p, 8, p, 4, ctypes.c_double(float("inf")), p, p, p, p, need, None) == -1 and b"thresh" in lib.car_last_error()
    assert lib.car_essential_ransac(p, p, 8, p, 4, th, p, p, p, p, need - 1, None) == -1 and b"workspace" in lib.car_last_error()
