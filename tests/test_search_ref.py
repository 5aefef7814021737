"""tests/search_ref.py, the numpy restatement of the search by projection, pinned on hand-made
cases without a GPU: the circle of rule L to the ulp, the lone candidate of rule N, what the gate is for (two equal
descriptors of which it sees one), the tie of rule M, positions that are not finite, and the states of rule P3-P5 with
the margin."""
import numpy as np

import reassoc_ref as R
import search_ref as S

OK = R.PD_OK
K = np.array([[100.0, 0.0, 50.0], [0.0, 100.0, 40.0], [0.0, 0.0, 1.0]])


def desc(byte, flips=0):
    d = np.full(32, byte, np.uint8)
    for b in range(flips):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def run(qdesc, qxy, tdesc, txy, qstate=None, tstate=None, tpstate=None, **kw):
    qstate = [OK] * len(qdesc) if qstate is None else qstate
    tstate = [OK] * len(tdesc) if tstate is None else tstate
    return S.reassociate_gated_window(np.array(qdesc), np.array(qstate), np.array(qxy, np.float32), np.array(tdesc),
                                      np.array(tstate), np.array(txy, np.float64), tpstate, **kw)


def test_a_pair_on_the_circle_is_a_candidate_and_one_ulp_outside_is_not():
    q, far = (10.0, 20.0), (400.0, 400.0)
    on = (10.0 + 3.0, 20.0 + 4.0)  # 3-4-5: exactly on the circle of radius 5
    out = (float(np.nextafter(13.0, np.inf)), 24.0)
    inn = (float(np.nextafter(13.0, -np.inf)), 24.0)
    for at, want in ((on, 2), (inn, 2), (out, 1)):
        # (a second train slot right at the query, so that the ratio test has its second neighbour)
        origin, dist, count, cand = run([desc(7)], [q], [desc(7), desc(9, 100), desc(1)], [at, q, far], radius_px=5.0,
                                        ratio=0.8)
        assert cand.tolist() == [want] and origin.tolist() == ([0] if want == 2 else [-1]), (at, origin, cand)
    assert S.gate_candidates(q, [on, out, inn], 5.0).tolist() == [True, False, True]
    # the test is on the float query widened to double, not on a double query
    qf = np.float32(0.1)
    assert S.gate_candidates((qf, 0.0), [(float(qf) - 5.0, 0.0), (0.1 - 5.0, 0.0)], 5.0).tolist() == [True, False]


def test_a_lone_candidate_under_both_values_of_accept_lone():
    args = ([desc(7, 3)], [(10.0, 10.0)], [desc(7), desc(7)], [(12.0, 10.0), (200.0, 10.0)])
    for lone, max_distance, want in ((0, 256, -1), (1, 256, 0), (1, 3, 0), (1, 2, -1)):
        origin, dist, count, cand = run(*args, radius_px=4.0, accept_lone=lone, max_distance=max_distance)
        assert cand.tolist() == [1] and origin.tolist() == [want] and count == (want >= 0), (lone, max_distance)
        assert dist.tolist() == ([3] if want >= 0 else [-1])
    # without candidates nothing is accepted, whatever accept_lone is
    origin, _, count, cand = run(*args, radius_px=1.0, accept_lone=1)
    assert cand.tolist() == [0] and origin.tolist() == [-1] and count == 0


def test_of_two_equal_descriptors_the_gate_sees_one():
    """the reason for the feature: d1 == d2 fails the ratio; inside the gate the twin is no candidate"""
    tdesc, txy = [desc(7), desc(7), desc(200, 9)], [(10.0, 10.0), (300.0, 10.0), (14.0, 10.0)]
    qd, qxy = [desc(7, 2)], [(11.0, 11.0)]
    plain = R.reassociate_window(np.array(qd), np.array([OK]), np.array(tdesc), np.array([OK] * 3), 0.8, 256, 1)
    assert plain[0].tolist() == [-1] and plain[2] == 0
    origin, dist, count, cand = run(qd, qxy, tdesc, txy, radius_px=10.0)
    assert cand.tolist() == [2] and origin.tolist() == [0] and dist.tolist() == [2] and count == 1
    # a circle over both twins is the ungated call
    origin, _, count, cand = run(qd, qxy, tdesc, txy, radius_px=1000.0)
    assert cand.tolist() == [3] and origin.tolist() == [-1] and count == 0


def test_a_tie_on_distance_inside_the_gate_goes_to_the_lower_slot():
    tdesc = [desc(1), desc(7, 1), desc(7, 1), desc(7, 1)]
    txy = [(0.0, 0.0), (52.0, 50.0), (49.0, 50.0), (500.0, 50.0)]
    origin, dist, count, cand = run([desc(7)], [(50.0, 50.0)], tdesc, txy, radius_px=5.0, ratio=1.0)
    assert cand.tolist() == [2] and origin.tolist() == [-1]  # d1 == d2 == 1: 1 < 1.0 * 1 fails
    origin, dist, count, cand = run([desc(7)], [(50.0, 50.0)], tdesc, txy, radius_px=5.0, ratio=1.5)
    assert origin.tolist() == [1] and dist.tolist() == [1]  # slot 1 before slot 2, though slot 2 is the nearer place
    # unique: the nearer of two queries keeps the slot, on a tie the lower query
    origin, dist, count, _ = run([desc(7, 2), desc(7, 1), desc(7, 1)], [(50.0, 50.0)] * 3,
                                 [desc(7), desc(99, 77)], [(51.0, 50.0), (50.0, 51.0)], radius_px=5.0, unique=1)
    assert origin.tolist() == [-1, 0, -1] and dist.tolist() == [-1, 1, -1] and count == 1


def test_positions_that_are_not_finite_and_states():
    tdesc, txy = [desc(7), desc(7), desc(7), desc(7)], [(np.nan, 10.0), (10.0, np.inf), (10.0, 10.0), (11.0, 10.0)]
    origin, _, _, cand = run([desc(7, 1)] * 3, [(10.0, 10.0), (np.nan, 10.0), (10.0, -np.inf)], tdesc, txy,
                             radius_px=3.0, ratio=1.0, unique=0)
    assert cand.tolist() == [2, 0, 0] and origin.tolist() == [-1, -1, -1]  # (slots 2 and 3 tie at d = 1)
    origin, _, _, cand = run([desc(7, 1)], [(10.0, 10.0)], tdesc, txy, radius_px=3.0, accept_lone=1,
                             tpstate=np.array([S.PROJ_OK, S.PROJ_OK, S.PROJ_OUTSIDE, S.PROJ_OK]))
    assert cand.tolist() == [1] and origin.tolist() == [3]
    origin, _, _, cand = run([desc(7, 1)], [(10.0, 10.0)], tdesc, txy, radius_px=3.0, accept_lone=1,
                             tstate=[OK, OK, OK, R.PD_BORDER])
    assert cand.tolist() == [1] and origin.tolist() == [2]
    origin, _, _, cand = run([desc(7, 1)], [(10.0, 10.0)], tdesc, txy, radius_px=3.0, accept_lone=1,
                             qstate=[R.PD_NONE])
    assert cand.tolist() == [0] and origin.tolist() == [-1]


def test_behind_outside_and_the_margin():
    pts = np.array([[0.0, 0.0, 2.0],      # slot 0: the principal point
                    [0.0, 0.0, -2.0],     # slot 2: behind
                    [0.0, 0.0, 0.0],      # slot 3: depth 0 is behind
                    [-1.0390625, 0.0, 2.0],  # slot 5: u = -1.953125, inside the margin of 2 only
                    [-1.0402, 0.0, 2.0],  # slot 6: u = -2.01
                    [1.0, 0.8, 2.0],      # slot 7: u = 100, v = 80: the far corner of a 99 x 79 frame with margin 2
                    [np.nan, 0.0, 2.0],   # slot 8: no landmark
                    [0.5, 0.5, 2.0]])     # slot 9
    slots = np.array([0, 2, 3, 5, 6, 7, 8, 9])
    ident = np.zeros(6)
    xy, depth, state, count = S.project_window(pts, slots, True, ident, K, 99, 79, 2.0, 11)
    N, B, O, G = S.PROJ_NONE, S.PROJ_BEHIND, S.PROJ_OUTSIDE, S.PROJ_OK
    assert state.tolist() == [G, N, B, B, N, G, O, G, N, G, N] and count == 4
    assert xy[0].tolist() == [50.0, 40.0] and depth[0] == 2.0 and xy[5].tolist() == [-1.953125, 40.0]
    assert np.allclose(xy[7], [100.0, 80.0], atol=1e-12) and xy[9].tolist() == [75.0, 65.0]
    assert not xy[state != G].any() and not depth[state != G].any()
    # without the margin slots 5 and 7 are outside
    _, _, state, count = S.project_window(pts, slots, True, ident, K, 99, 79, 0.0, 11)
    assert state.tolist() == [G, N, B, B, N, O, O, O, N, G, N] and count == 2
    # a quarter turn about y puts +x in front: Rodrigues by hand
    Rm = S.rodrigues([0.0, -np.pi / 2, 0.0])
    assert np.allclose(Rm, [[0, 0, -1], [0, 1, 0], [1, 0, 0]], atol=1e-15)
    xy, depth, state, _ = S.project_window([[3.0, 0.0, 0.0]], [1], True, [0.0, -np.pi / 2, 0.0, 0.0, 0.0, 1.0], K, 99,
                                           79, 0.0, 2)
    assert state.tolist() == [N, G] and np.allclose(xy[1], [50.0, 40.0], atol=1e-12) and np.isclose(depth[1], 4.0)
    # rule P2 and a window that is not OK
    for pose, ok in (([0.0, 1.1e5, 0.0, 0, 0, 0], True), ([0.0, 0.0, 0.0, np.inf, 0, 0], True), (ident, False)):
        xy, depth, state, count = S.project_window(pts, slots, ok, np.array(pose, float), K, 99, 79, 2.0, 11)
        assert count == 0 and not state.any() and not xy.any() and not depth.any()
    assert S.pose_accepted([0.0, 1.0e5, 0.0, 1, 2, 3]) and not S.pose_accepted([0.0, 1.0e5, 1.0, 1, 2, 3])


def test_the_scenes_are_what_they_are_there_for():
    for frame in ((96, 64), (1241, 40)):
        g = S.gated_windows(70, 300, frame, 41)
        ref = S.reassociate_gated(g["qdesc"], g["qstate"], g["qxy"], g["tdesc"], g["tstate"], g["txy"], g["tpstate"],
                                  radius_px=8.0, ratio=0.8, max_distance=256, accept_lone=1, unique=0)
        assert ref["count"][0] > 10 and ref["count"][1] > 5 and ref["count"][2] == 0 and not ref["candidates"][2].any()
        assert ref["candidates"][1].max() > 256  # the clump: more than 256 train slots inside one gate
        assert (ref["candidates"][0] == 0).any() and (ref["candidates"][0] >= 2).any()
    r = S.repeated_structure()
    n = len(r["right"])
    plain = R.reassociate(r["qdesc"], r["qstate"], r["tdesc"], r["tstate"], 0.8, 256, 1)
    assert plain["count"].tolist() == [0] and (plain["origin"] == -1).all()
    for lone in (0, 1):
        gated = S.reassociate_gated(r["qdesc"], r["qstate"], r["qxy"], r["tdesc"], r["tstate"], r["txy"],
                                    radius_px=10.0, ratio=0.8, max_distance=256, accept_lone=lone, unique=1)
        assert gated["count"].tolist() == [n] and gated["origin"][0].tolist() == r["right"].tolist()
        assert gated["candidates"][0].tolist() == [2] * n and gated["dist"][0].tolist() == [q % 7 for q in range(n)]
