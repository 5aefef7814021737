"""CPU-only checks of the PnP arithmetic: csrc/orbx_pnp_math.h through the sequential
restatement tests/cpp/pnp_sequential.cpp, against the independent numpy reference tests/pnp_ref.py and against the true
poses of synthetic scenes.

Measured here on the CPU (the rank-17 table):
  solver       500 seeded problems, 5 left out as near-degenerate (the cap is 10 = 2 %); the largest matched difference
               between a header solution and a reference solution is 4.24e-8 -> tolerance 4.3e-7
  true pose    40 noise-free scenes of 100 points, refine_iters 10: at most 1.25e-16 rad and 1.66e-15 units from the
               true pose (binary64 rounding of the scene itself) -> bounds 1.3e-15 rad, 1.7e-14 units
  outliers     40 scenes with 30 % of the observations displaced by 20 .. 100 px, threshold_px 2: every mask equals the
               true inlier set"""
import math

import numpy as np
import pytest

import pnp_ref as R
import pnp_seq as S
from landmarks_ref import K_KITTI as K

SOLVER_SEEDS = range(1000, 1500)
SOLVER_TOL = 4.3e-7     # 10 x 4.24e-8
SOLVER_CAP = 10         # 2 % of 500
POSE_TOL_ROT = 1.3e-15  # 10 x 1.25e-16 rad
POSE_TOL_T = 1.7e-14    # 10 x 1.66e-15 units
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def seq(tmp_path_factory):
    return S.compile_so(tmp_path_factory.mktemp("pnp_seq"))


def test_p3p_against_the_numpy_reference(seq):
    worst, left_out, solutions = 0.0, 0, 0
    for seed in SOLVER_SEEDS:
        X, xy, truth = R.p3p_problem(seed)
        ref, near = R.p3p(X, xy)
        if near:
            left_out += 1
            continue
        got = S.p3p(seq, X, xy)
        assert len(got) == len(ref) and len(ref) >= 1, (seed, len(got), len(ref))
        d = np.array([[R.solution_distance(g, r) for r in ref] for g in got])
        # every reference solution is matched by a header solution, and every header solution by a reference one
        assert d.min(0).max() <= SOLVER_TOL and d.min(1).max() <= SOLVER_TOL, (seed, d)
        # ascending v on both sides: the solutions come in the same order
        assert list(d.argmin(1)) == list(range(len(ref))), (seed, d)
        worst = max(worst, d.min(0).max(), d.min(1).max())
        solutions += len(ref)
        assert min(R.solution_distance(g, truth) for g in got) <= SOLVER_TOL, seed  # the true pose is among them
    print("largest matched difference %.3e, %d problems left out, %d solutions" % (worst, left_out, solutions))
    assert left_out <= SOLVER_CAP
    assert solutions > 1.5 * (len(SOLVER_SEEDS) - left_out)  # (problems with two and four solutions take part)


def test_p3p_degenerate_samples(seq):
    X, xy, _ = R.p3p_problem(7)
    line = np.array([X[0], X[0] + (X[1] - X[0]), X[0] + 2.5 * (X[1] - X[0])])
    assert S.p3p(seq, line, xy) == []  # collinear world points
    assert S.p3p(seq, np.array([X[0], X[0], X[2]]), xy) == []  # a repeated point
    assert S.p3p(seq, X * np.nan, xy) == []
    behind = S.p3p(seq, X, -xy)  # the mirrored bearings: whatever comes out has its sample in front of the camera
    for Rm, t in behind:
        assert np.all((X @ Rm.T + t)[:, 2] > 0)
    for Rm, t in S.p3p(seq, X, xy):
        assert abs(np.linalg.det(Rm) - 1.0) < 1e-9 and np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-9


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, it, k, n):
    h = mix64(seed ^ mix64((it << 32) | k))
    return ((h >> 32) * n) >> 32


def test_sampler_is_pose_samples_rule_with_three_indices(seq):
    idx = np.zeros(3, np.uint32)
    for seed, n in ((0, 4), (99, 5), (2 ** 63 + 5, 7), (12345, 1000)):
        for it in range(200):
            assert seq.seq_pnp_sample3(seed, it, n, idx.ctypes.data) == 1
            want, k = [], 0
            while len(want) < 3:
                v = draw(seed, it, k, n)
                k += 1
                if v not in want:
                    want.append(v)
            assert list(idx) == want, (seed, n, it)
    assert seq.seq_pnp_sample3(1, 0, 2, idx.ctypes.data) == 0  # three distinct indices below 2: the draws run out


def test_problem_seed_is_the_bindings(seq, pkg):
    for seed, k in ((0, 2), (7, 4), (2 ** 64 - 1, 7)):
        want = mix64(seed ^ mix64(k))
        assert seq.seq_pnp_problem_seed(seed, k) == want == pkg.orbx_pnp.problem_seed(seed, k)


def test_update_niters_has_exponent_three(seq):
    for p, ep, cap in ((0.99, 0.3, 1000), (0.999, 0.5, 1000), (0.99, 0.9, 100000), (0.99, 0.0, 1000), (0.5, 0.7, 10)):
        want = math.log(1 - p) / math.log(1 - (1 - ep) ** 3) if ep > 0 else 0
        got = seq.seq_pnp_update_niters(p, ep, cap)
        assert got == min(cap, int(round(want))) or abs(got - want) <= 0.5 + 1e-9, (p, ep, got, want)
    assert seq.seq_pnp_update_niters(0.99, 1.0, 50) == 50
    assert seq.seq_pnp_update_niters(0.99, 0.3, 1000) == 11


def test_true_pose_noise_free(seq):
    worst = [0.0, 0.0]
    for seed in range(2000, 2040):
        X, uv, (Rt, tt), _ = R.scene(seed, n=100)
        r = S.problem(seq, K, X, uv, refine_iters=10, seed=seed)
        assert r["status"] == S.OK and r["inliers"] == r["n_corr"] == 100 and r["mask"].all()
        er, et = R.pose_error(r["pose6"], Rt, tt)
        worst = [max(worst[0], er), max(worst[1], et)]
        assert er <= POSE_TOL_ROT and et <= POSE_TOL_T, (seed, er, et)
        assert r["rms_px"] < 1e-9
    print("worst: %.3e rad, %.3e units" % tuple(worst))


def test_outliers_are_masked_exactly(seq):
    for seed in range(3000, 3040):
        X, uv, (Rt, tt), inl = R.scene(seed, n=100, outliers=0.3)
        assert inl.sum() == 70
        r = S.problem(seq, K, X, uv, refine_iters=10, seed=seed, threshold_px=2.0)
        assert r["status"] == S.OK and np.array_equal(r["mask"].astype(bool), inl), seed
        assert r["inliers"] == 70 and 3 <= r["iters"] < 100
        er, et = R.pose_error(r["pose6"], Rt, tt)
        assert er <= POSE_TOL_ROT and et <= POSE_TOL_T, (seed, er, et)


def test_statuses_and_limits(seq):
    X, uv, (Rt, tt), _ = R.scene(11, n=60)
    few = S.problem(seq, K, X[:3], uv[:3])
    assert (few["status"], few["n_corr"], few["inliers"], few["iters"]) == (S.FEW_POINTS, 3, 0, 0)
    assert not few["mask"].any() and not few["pose6"].any()
    assert S.problem(seq, K, X[:9], uv[:9], min_inliers=10)["status"] == S.FEW_POINTS
    none = S.problem(seq, K, X, uv, max_iters=0)
    assert (none["status"], none["iters"], none["inliers"]) == (S.NO_MODEL, 0, 0)
    rng = np.random.default_rng(3)
    junk = S.problem(seq, K, X, np.c_[rng.uniform(0, 1241, 60), rng.uniform(0, 376, 60)], max_iters=200,
                     threshold_px=0.5, min_inliers=6)
    assert (junk["status"], junk["iters"]) == (S.NO_MODEL, 200) and not junk["mask"].any()
    # min_inliers is a floor on the best model: 12 consistent points among 60 pass 12 and fail 13
    mixed = np.c_[rng.uniform(0, 1241, 60), rng.uniform(0, 376, 60)]
    mixed[:12] = uv[:12]
    ok = S.problem(seq, K, X, mixed, max_iters=5000, min_inliers=12, seed=5)
    assert ok["status"] == S.OK and ok["inliers"] == 12 and ok["mask"][:12].all() and not ok["mask"][12:].any()
    assert S.problem(seq, K, X, mixed, max_iters=5000, min_inliers=13, seed=5)["status"] == S.NO_MODEL
    zero = S.problem(seq, K, X, uv, threshold_px=0.0, refine_iters=0)  # e2 <= 0: only exact reprojections
    assert zero["status"] in (S.OK, S.NO_MODEL) and zero["inliers"] == int(zero["mask"].sum())


def test_refinement_never_loses_inliers(seq):
    """noisy pixels: the refined pose is kept only with at least the RANSAC pose's inliers, and lowers the RMS when
    the inlier set is the same"""
    rng = np.random.default_rng(8)
    for seed in range(4000, 4010):
        X, uv, (Rt, tt), _ = R.scene(seed, n=150)
        uv = uv + rng.normal(0.0, 0.5, uv.shape)
        r0 = S.problem(seq, K, X, uv, refine_iters=0, seed=seed, threshold_px=2.0)
        r1 = S.problem(seq, K, X, uv, refine_iters=20, seed=seed, threshold_px=2.0)
        assert r0["status"] == r1["status"] == S.OK and r0["iters"] == r1["iters"]
        assert r1["inliers"] >= r0["inliers"] > 100
        if np.array_equal(r0["mask"], r1["mask"]):
            assert r1["rms_px"] <= r0["rms_px"]
        e0, e1 = R.pose_error(r0["pose6"], Rt, tt), R.pose_error(r1["pose6"], Rt, tt)
        assert e1[0] < 5e-3 and e1[1] < 0.1, (seed, e0, e1)


def test_batch_on_a_landmarks_block(seq):
    """the gather of seq_pnp_windows on a block in the format of Context.landmarks_fetch equals seq_pnp_problem on the
    observations of frame k picked by hand"""
    import landmarks_ref as L
    import landmarks_seq as LS

    lm = LS.compile_so(__import__("pathlib").Path(seq._name).parent, "lm_sequential")
    scenes = [L.make_scene(61, W=5, slots=65, min_seen=0), L.make_scene(62, W=5, slots=65, min_seen=2)]
    scenes[1]["poses"][1, 3:] = scenes[1]["poses"][0, 3:]  # no baseline: not OK
    poses, tracks, seen = L.stack(scenes)
    block = LS.seq_build(lm, K, poses, tracks, seen)
    assert list(block["status"]) == [L.OK, L.BASELINE]
    got = S.windows(seq, K, block, poses, 65, seed=9)
    assert (got["records"]["status"][1] == S.SKIPPED).all() and not got["mask"][1].any()
    assert np.array_equal(got["poses6"][1], poses[1]) and np.array_equal(got["poses6"][0, :2], poses[0, :2])
    pts, _, op, oq, xy = LS.window_of(block, 0)
    for k in (2, 3, 4):
        sel = oq == k
        one = S.problem(seq, K, pts[op[sel]], xy[sel], seed=seq.seq_pnp_problem_seed(9, k))
        rec = got["records"][0, k - 2]
        assert rec["n_corr"] == sel.sum() == (scenes[0]["seen"][block["slot_of_point"][:len(pts)]] > k).sum()
        assert rec["status"] == one["status"] == S.OK
        assert rec["pose6"].tobytes() == one["pose6"].tobytes() == got["poses6"][0, k].tobytes()
        assert (rec["inliers"], rec["iters"], rec["rms_px"]) == (one["inliers"], one["iters"], one["rms_px"])
        mask = np.zeros(65, np.uint8)
        mask[op[sel]] = one["mask"]
        assert np.array_equal(got["mask"][0, k - 2], mask)
        er, et = R.pose_error(rec["pose6"], L.rodrigues(scenes[0]["true_poses"][k, :3]), scenes[0]["true_poses"][k, 3:])
        assert er < 1e-4 and et < 1e-2  # float32 pixels: the true pose up to their rounding
