"""Landmarks of tracked windows (the reference's buildLandmarksFromFirstTwoFramesAndTracks,
src/with_bundle_adjustment.cpp:502-575): the sequential restatement tests/cpp/lm_sequential.cpp, which shares
orbx_lm_math.h with the kernels, against known answers and against the independent numpy restatement
tests/landmarks_ref.py (numpy.linalg.svd).  No GPU.  The GPU tests (tests/test_landmarks.py) pin the kernels bit for
bit to the same restatement.  Measured worst cases are tabulated in DESIGN.md §9 rank 10."""
import numpy as np
import pytest

import landmarks_ref as R
import landmarks_seq as S

K = R.K_KITTI
# Restatement (Jacobi sweeps on the 4 x 4 normal matrix) against numpy's SVD of the system itself, points with at
# least 1 degree of parallax: the worst relative point difference measured over the scenes of
# test_restatement_matches_numpy_svd was 2.32e-12 (noiseless) and 2.01e-12 (sigma = 0.3 px); the bound is 100 x the
# larger one, the margin DESIGN.md §9 rank 7 gives its Schur step (rounding-level quantities move by orders of
# magnitude between seeds).
SVD_REL_BOUND = 2.32e-10


@pytest.fixture(scope="module")
def seq(tmp_path_factory):
    return S.compile_so(tmp_path_factory.mktemp("lm_seq"), "lm_sequential")


@pytest.fixture(scope="module")
def ba_seq(tmp_path_factory):
    return S.compile_so(tmp_path_factory.mktemp("lm_ba_seq"), "ba_sequential")


def build_one(seq, scene):
    return S.seq_build(seq, K, *R.stack([scene]))


def test_header_and_restatement_agree_on_the_status_values(pkg):
    o = pkg.orbx
    assert (o.LM_OK, o.LM_BASELINE, o.LM_EMPTY, o.LM_BAD_POSE) == (R.OK, R.BASELINE, R.EMPTY, R.BAD_POSE) == (0, 1, 2, 3)
    assert o.BA_SKIPPED == 3
    for name in ("landmarks_build", "landmarks_view", "landmarks_fetch", "bundle_adjust_landmarks",
                 "bundle_adjust_landmarks_fetch", "bundle_adjust_tracks"):
        assert hasattr(pkg.Context, name), name


def test_known_answers_on_a_noiseless_scene(seq):
    """Every point in front of both cameras, seen at least twice and with world z > 0 is kept, in slot order, with its
    `seen` observations; world z <= 0 is dropped although the point is in front of the cameras; seen 0 / 1 never
    appears."""
    sc = R.make_scene(11, W=5, slots=600, world=R.WORLD_TILTED)
    out = build_one(seq, sc)
    assert out["status"][0] == R.OK
    pts, slot, op, oq, xy = S.window_of(out, 0)
    z, norm = sc["X"][:, 2], np.linalg.norm(sc["X"], axis=1)
    # the pixels are float32: a point within 1e-3 |X| of the plane z = 0 may fall on either side
    decided = np.abs(z) > 1e-3 * norm
    want = (sc["seen"] >= 2) & (z > 0)
    got = np.zeros(len(z), bool)
    got[slot] = True
    assert np.array_equal(got[decided], want[decided])
    assert np.all(sc["seen"][slot] >= 2)
    dropped_in_front = (sc["seen"] >= 2) & (z < -1e-3 * norm)
    assert dropped_in_front.sum() > 20 and not got[dropped_in_front].any()
    assert got.sum() > 200
    assert np.all(np.diff(slot) > 0)  # slot order
    # float32 pixels: half an ulp at 1241 px is 6e-5 px in each of two frames; the relative depth error of a point
    # with parallax p is about (pixel error) / (f p), 1e-5 at one degree -- bounded with a margin of 10
    good = sc["parallax"][slot] >= 1.0
    err = np.linalg.norm(pts - sc["X"][slot], axis=1) / np.linalg.norm(sc["X"][slot] - sc_centre0(sc), axis=1)
    assert good.sum() > 50 and err[good].max() < 1e-4, err[good].max()
    # observations: k = 0 .. seen - 1 of the slot, the float pixels widened
    assert out["obs_offset"][1] == sc["seen"][slot].sum() == len(op)
    at = 0
    for j, s in enumerate(slot):
        n = sc["seen"][s]
        assert np.array_equal(op[at:at + n], np.full(n, j)) and np.array_equal(oq[at:at + n], np.arange(n))
        assert np.array_equal(xy[at:at + n], sc["tracks"][s, :n].astype(np.float64))
        at += n


def sc_centre0(sc):
    p = sc["true_poses"][0]
    return -R.rodrigues(p[:3]).T @ p[3:]


def gate_window(b, axis):
    """Two identity rotations, t0 = 0 and t1 = b along one axis: t0 - t1 is b to the bit and the root of b * b is
    exact.  One point in front of both cameras, off every axis."""
    poses = np.zeros((1, 2, 6))
    poses[0, 1, 3 + axis] = b
    tracks = np.zeros((1, 1, 2, 2), np.float32)
    X = np.array([3.0, -2.0, 50.0])
    for k in range(2):
        p = X + poses[0, k, 3:]
        tracks[0, 0, k] = (K[0, 0] * p[0] / p[2] + K[0, 2], K[1, 1] * p[1] / p[2] + K[1, 2])
    return poses, tracks, np.full((1, 1), 2, np.int32)


@pytest.mark.parametrize("b,want", [(0.0999, R.BASELINE), (0.1, R.OK), (100.0, R.OK), (100.001, R.BASELINE)])
def test_baseline_gate(seq, b, want):
    for axis in range(3):
        for sign in (1.0, -1.0):
            poses, tracks, seen = gate_window(sign * b, axis)
            got = S.seq_build(seq, K, poses, tracks, seen)
            assert got["status"][0] == want, (b, axis, sign)
            assert got["point_offset"][1] == (1 if want == R.OK else 0)
            assert R.np_build(K, poses[0], tracks[0], seen[0])[0] == want


def test_bad_pose_and_empty(seq):
    sc = R.make_scene(3, W=3, slots=50, min_seen=2)
    bad = dict(sc, poses=sc["poses"].copy())
    bad["poses"][1, :3] = np.array([2e5, 0.0, 0.0])  # theta = 2e5 > BA_MAX_THETA
    out = build_one(seq, bad)
    assert out["status"][0] == R.BAD_POSE and out["point_offset"][1] == 0 and out["obs_offset"][1] == 0
    assert R.np_build(K, bad["poses"], bad["tracks"], bad["seen"])[0] == R.BAD_POSE
    behind = R.make_scene(4, W=3, slots=50, min_seen=2, depth_sign=-1.0)
    out = build_one(seq, behind)
    assert out["status"][0] == R.EMPTY and out["point_offset"][1] == 0 and out["obs_offset"][1] == 0
    assert R.np_build(K, behind["poses"], behind["tracks"], behind["seen"])[0] == R.EMPTY


SVD_SCENES = [(21, 5, 0.0), (22, 5, 0.0), (23, 8, 0.0), (24, 2, 0.0), (31, 5, 0.3), (32, 5, 0.3), (33, 8, 0.3),
              (34, 2, 0.3)]


def test_restatement_matches_numpy_svd(seq):
    """Worst relative point difference against numpy.linalg.svd (the independent reference) over points with at least
    one degree of parallax, printed per noise level; the keep / drop decision agrees wherever |z| exceeds the bound
    times |X|."""
    worst = {0.0: 0.0, 0.3: 0.0}
    compared = 0
    for seed, W, sigma in SVD_SCENES:
        for world in (R.WORLD_TILTED, (R.rodrigues(np.array([0.4, -1.1, 0.7])), np.array([3.0, -7.0, 11.0]))):
            sc = R.make_scene(seed, W=W, slots=400, sigma=sigma, world=world)
            out = build_one(seq, sc)
            pts, slot, _, _, _ = S.window_of(out, 0)
            st, npts, nslot, _, _, _ = R.np_build(K, sc["poses"], sc["tracks"], sc["seen"])
            assert st == out["status"][0] == R.OK
            ok = sc["parallax"] >= 1.0
            both = np.intersect1d(slot, nslot)
            both = both[ok[both]]
            a = pts[np.searchsorted(slot, both)]
            b = npts[np.searchsorted(nslot, both)]
            rel = np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)
            worst[sigma] = max(worst[sigma], float(rel.max()))
            compared += len(both)
            # keep / drop: a slot only one side kept has |z| within the bound of the plane (numpy's value decides),
            # or too little parallax to be compared at all
            for s in np.setxor1d(slot, nslot):
                if not ok[s]:
                    continue
                if s in nslot:
                    X = npts[np.searchsorted(nslot, s)]
                else:
                    X = pts[np.searchsorted(slot, s)]
                assert abs(X[2]) <= SVD_REL_BOUND * np.linalg.norm(X), (seed, s, X)
    print("restatement vs numpy SVD, worst relative point difference: noiseless %.3g, sigma 0.3 px %.3g (%d points)"
          % (worst[0.0], worst[0.3], compared))
    assert compared > 1000
    assert max(worst.values()) <= SVD_REL_BOUND, worst


def test_layout_is_what_the_solver_accepts(seq, ba_seq):
    """The fetched-format arrays of the restatement: rows monotone, every (landmark, pose) at most once, and
    ba_sequential solves the window."""
    sc = R.make_scene(41, W=5, slots=300, min_seen=0, world=R.WORLD_TILTED, pose_pert=0.002)
    out = build_one(seq, sc)
    pts, slot, op, oq, xy = S.window_of(out, 0)
    assert len(pts) > 100
    assert np.all(np.diff(op) >= 0) and op[0] == 0 and op[-1] == len(pts) - 1  # rows are monotone and complete
    key = op.astype(np.int64) * 5 + oq
    assert len(np.unique(key)) == len(key) and oq.min() == 0 and oq.max() <= 4
    assert np.all(np.diff(out["point_offset"]) >= 0) and np.all(np.diff(out["obs_offset"]) >= 0)
    poses, pts2, s = S.seq_ba(ba_seq, K, sc["poses"], pts, op, oq, xy)
    assert s["termination"] == 0 and s["final_cost"] <= s["initial_cost"] and s["iterations"] >= 1
    # the refined poses are nearer to the truth than the perturbed start
    assert np.abs(poses[2:] - sc["true_poses"][2:]).max() < np.abs(sc["poses"][2:] - sc["true_poses"][2:]).max()
