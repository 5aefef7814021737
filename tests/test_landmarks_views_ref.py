"""Landmarks from every view of a track with a reprojection gate (include/orbx_lm.h): the
sequential restatement tests/cpp/lm_views_sequential.cpp, which shares orbx_lm_math.h with the kernels, against the
independent numpy restatement tests/landmarks_views_ref.py (numpy.linalg.svd), and the conditions the feature is there
for: points of less than 0.6 times the error of the first-two build at W = 5, moved observations rejected, in-front
points kept whatever the world frame.  No GPU.  The GPU tests (tests/test_landmarks_views.py) pin the kernels bit for
bit to the same restatement.  Measured worst cases are tabulated in DESIGN.md §9 rank 15."""
import numpy as np
import pytest

import landmarks_ref as R
import landmarks_seq as S
import landmarks_views_ref as V
import landmarks_views_seq as VS

K = R.K_KITTI
# Restatement (Jacobi sweeps on the 4 x 4 normal matrix summed over the views) against numpy's SVD of the 2 m x 4 system
# itself, points with at least 1 degree of parallax between views 0 and 1: the worst relative point difference measured
# over the scenes and modes of test_restatement_matches_numpy_svd was 2.69e-12; the bound is 100 x that, rank 10's
# convention.
SVD_REL_BOUND = 2.69e-10
# reason has to be equal wherever the decision is not marginal: the largest error further than this (relative) from
# the threshold, the smallest depth further than this (relative to the point's distance) from 0
MARGIN = 1e-6
OTHER_WORLD = (R.rodrigues(np.array([0.4, -1.1, 0.7])), np.array([3.0, -7.0, 11.0]))


@pytest.fixture(scope="module")
def seq(tmp_path_factory):
    return S.compile_so(tmp_path_factory.mktemp("lm_views_seq"), "lm_views_sequential")


def build_one(seq, sc, mode, gate):
    out, reason, px = VS.seq_views_build(seq, K, *R.stack([sc]), mode, gate)
    return out, reason[0], px[0]


def compare(seq, sc, mode, gate):
    """One scene through both restatements: reason equal wherever numpy's decision is not marginal (the count of
    marginal slots is returned and bounded by the caller), the points of numpy's kept slots with parallax within
    SVD_REL_BOUND.  Returns (worst relative difference, points compared, marginal slots)."""
    out, reason, px = build_one(seq, sc, mode, gate)
    ref = V.np_build_views(K, sc["poses"], sc["tracks"], sc["seen"], mode, gate)
    assert out["status"][0] == ref["status"]
    marginal = np.zeros(len(reason), bool)
    if gate > 0:
        marginal |= np.abs(ref["max_e2"] - gate * gate) <= MARGIN * gate * gate
    with np.errstate(invalid="ignore"):
        marginal |= np.abs(ref["min_depth"]) <= MARGIN * 40.0  # (the points lie within 40 units of camera 0)
    assert np.array_equal(reason[~marginal], ref["reason"][~marginal]), (mode, gate)
    finite = np.isfinite(ref["reproj_px"]) & ~marginal
    assert np.array_equal(np.isfinite(px), np.isfinite(ref["reproj_px"]))
    # reproj_px is a float32 of a value that differs by the points' difference: compared loosely, in pixels
    assert np.allclose(px[finite], ref["reproj_px"][finite], rtol=1e-4, atol=1e-4)
    pts, slot, _, _, _ = S.window_of(out, 0)
    both = np.intersect1d(slot, ref["slot_of_point"])
    both = both[sc["parallax"][both] >= 1.0]
    a = pts[np.searchsorted(slot, both)]
    b = ref["points"][np.searchsorted(ref["slot_of_point"], both)]
    rel = np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)
    return (float(rel.max()) if len(rel) else 0.0), len(both), int(marginal.sum())


SVD_SCENES = [(21, 5, 0.0), (23, 8, 0.0), (24, 2, 0.0), (25, 3, 0.0), (31, 5, 0.3), (33, 8, 0.3), (34, 2, 0.3),
              (35, 3, 0.3)]


def test_restatement_matches_numpy_svd(seq):
    worst, compared, marginal = 0.0, 0, 0
    for seed, W, sigma in SVD_SCENES:
        for world in (R.WORLD_TILTED, OTHER_WORLD):
            sc = R.make_scene(seed, W=W, slots=200, sigma=sigma, world=world, outliers=0.1 if sigma else 0.0)
            for mode in VS.MODES:
                for gate in (0.0, 3.0):
                    w, n, m = compare(seq, sc, mode, gate)
                    worst, compared, marginal = max(worst, w), compared + n, marginal + m
    print("views restatement vs numpy SVD, worst relative point difference %.3g (%d points, %d marginal decisions "
          "excluded)" % (worst, compared, marginal))
    assert compared > 4000 and marginal <= 5
    assert worst <= SVD_REL_BOUND, worst


def test_two_observations_give_one_point_in_every_mode(seq):
    sc = R.make_scene(51, W=5, slots=300, sigma=0.3, world=OTHER_WORLD)
    two = np.flatnonzero(sc["seen"] == 2)
    assert len(two) > 30
    pts = []
    for mode in VS.MODES:
        out, reason, _ = build_one(seq, sc, mode, 0.0)
        p, slot, _, _, _ = S.window_of(out, 0)
        kept = np.isin(two, slot)
        assert kept.sum() > 15 and np.all(reason[two[kept]] == V.KEPT)
        pts.append((two[kept], p[np.searchsorted(slot, two[kept])]))
    for slots, p in pts[1:]:
        # (first-two judges by world z, the others by camera depth: the kept sets may differ, the points may not)
        common = np.intersect1d(slots, pts[0][0])
        assert len(common) > 15
        a = pts[0][1][np.searchsorted(pts[0][0], common)]
        b = p[np.searchsorted(slots, common)]
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def median_error(seq, scenes, mode):
    err = []
    for sc in scenes:
        out, _, _ = build_one(seq, sc, mode, 0.0)
        pts, slot, _, _, _ = S.window_of(out, 0)
        err.append(np.linalg.norm(pts - sc["X"][slot], axis=1) / np.linalg.norm(sc["X"][slot], axis=1))
    return float(np.median(np.concatenate(err)))


def test_more_views_give_better_points(seq):
    """the issue's accuracy condition: at W = 5 the median relative point error of ALL_VIEWS and of WIDEST is each
    below 0.6 x FIRST_TWO's (numpy: 0.43 and 0.44); at W = 3 it is merely below it"""
    for W, factor in ((5, 0.6), (3, 1.0)):
        scenes = [R.make_scene(seed, W=W, slots=200, sigma=0.3, min_seen=2) for seed in range(4)]
        e = [median_error(seq, scenes, mode) for mode in VS.MODES]
        print("W = %d: median relative error first two %.4g, widest %.4g (x %.2f), all views %.4g (x %.2f)"
              % (W, e[0], e[1], e[1] / e[0], e[2], e[2] / e[0]))
        assert e[1] < factor * e[0] and e[2] < factor * e[0], (W, e)


def test_the_gate_rejects_moved_observations(seq):
    """the issue's gate condition: outliers = 0.2, 3 px, W = 5 -- at least 95 % of the tracks with a moved observation
    are REPROJECTION and no clean track is (numpy: 225 / 226 and 0 / 574)"""
    moved_total = moved_hit = clean_total = clean_hit = 0
    closest = np.inf
    for seed in range(4):
        kw = dict(W=5, slots=200, sigma=0.3, min_seen=2)
        sc, clean = R.make_scene(seed, outliers=0.2, **kw), R.make_scene(seed, **kw)
        assert np.array_equal(sc["seen"], clean["seen"])
        moved = np.any(sc["tracks"] != clean["tracks"], axis=(1, 2))
        _, reason, px = build_one(seq, sc, V.ALL_VIEWS, 3.0)
        ref = V.np_build_views(K, sc["poses"], sc["tracks"], sc["seen"], V.ALL_VIEWS, 3.0)
        assert np.array_equal(reason, ref["reason"])
        assert np.all(reason[~moved] == V.KEPT)
        moved_total, moved_hit = moved_total + moved.sum(), moved_hit + (reason[moved] == V.REPROJECTION).sum()
        clean_total, clean_hit = clean_total + (~moved).sum(), clean_hit + (reason[~moved] == V.REPROJECTION).sum()
        closest = min(closest, float(np.abs(px - 3.0).min()))
    print("gate at 3 px: %d of %d moved tracks rejected, %d of %d clean ones; closest decision %.3g px from it"
          % (moved_hit, moved_total, clean_hit, clean_total, closest))
    assert moved_total > 150 and moved_hit >= 0.95 * moved_total and clean_hit == 0


def test_a_tilted_world_keeps_the_points_in_front(seq):
    """WORLD_TILTED: about a fifth of the points in front of every camera has world z <= 0; FIRST_TWO drops them,
    ALL_VIEWS keeps them"""
    sc = R.make_scene(11, W=5, slots=600, world=R.WORLD_TILTED, min_seen=2)
    _, first, _ = build_one(seq, sc, V.FIRST_TWO, 0.0)
    _, allv, _ = build_one(seq, sc, V.ALL_VIEWS, 0.0)
    z, norm = sc["X"][:, 2], np.linalg.norm(sc["X"], axis=1)
    below = z < -1e-3 * norm
    assert below.sum() > 60 and np.all(first[below] == V.BEHIND) and np.all(allv[below] == V.KEPT)
    assert np.all(allv == V.KEPT) and (first == V.KEPT).sum() < 0.9 * len(z)


def test_reasons_of_a_mixed_window(seq):
    """SHORT, BEHIND and NO_WINDOW with their reproj_px; a bad pose beyond view 1 counts in every case but FIRST_TWO
    without a gate"""
    sc = R.make_scene(61, W=5, slots=100, min_seen=0)
    behind = R.make_scene(62, W=5, slots=100, min_seen=0, depth_sign=-1.0)
    for mode in VS.MODES:
        for gate in (0.0, 3.0):
            out, reason, px = build_one(seq, sc, mode, gate)
            assert out["status"][0] == R.OK
            assert np.array_equal(reason == V.SHORT, sc["seen"] < 2) and np.all(px[reason == V.SHORT] == 0)
            assert np.all(reason[sc["seen"] >= 2] == V.KEPT)
            out, reason, px = build_one(seq, behind, mode, gate)
            assert out["status"][0] == R.EMPTY and set(reason) == {V.SHORT, V.BEHIND}
            bad = dict(sc, poses=sc["poses"].copy())
            bad["poses"][3, :3] = np.array([0.0, 2e5, 0.0])
            out, reason, px = build_one(seq, bad, mode, gate)
            if mode == V.FIRST_TWO and gate == 0.0:
                assert out["status"][0] == R.OK
            else:
                assert out["status"][0] == R.BAD_POSE and np.all(reason == V.NO_WINDOW) and np.all(px == 0)
            ref = V.np_build_views(K, bad["poses"], bad["tracks"], bad["seen"], mode, gate)
            assert ref["status"] == out["status"][0] and np.array_equal(ref["reason"], reason)


def test_an_observation_that_is_not_finite(seq):
    """reproj_px is +inf to the bit, the landmark falls to the gate only when there is one"""
    sc = R.make_scene(63, W=5, slots=50, min_seen=5)
    sc["tracks"][7, 3, 0] = np.inf
    for gate, want in ((0.0, V.KEPT), (3.0, V.REPROJECTION)):
        _, reason, px = build_one(seq, sc, V.WIDEST, gate)  # (views 0 and 4 make the point, view 3 only judges it)
        assert reason[7] == want and px.view(np.uint32)[7] == 0x7F800000
        assert np.all(reason[np.arange(50) != 7] == V.KEPT)


def test_first_two_without_a_gate_is_the_build_of_rank_10(seq, tmp_path_factory):
    old = S.compile_so(tmp_path_factory.mktemp("lm_seq_old"), "lm_sequential")
    scenes = [R.make_scene(71, W=5, slots=257, min_seen=0, world=R.WORLD_TILTED, sigma=0.3, outliers=0.1),
              R.make_scene(72, W=5, slots=257, min_seen=0, depth_sign=-1.0)]
    got, _, _ = VS.seq_views_build(seq, K, *R.stack(scenes), V.FIRST_TWO, 0.0)
    S.assert_blocks_equal(got, S.seq_build(old, K, *R.stack(scenes)))
