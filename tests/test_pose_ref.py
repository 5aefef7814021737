"""The relative-pose arithmetic of csrc/orbx_pose_math.h (through the exports of tests/cpp/pose_sequential.cpp)
against tests/pose_ref.py, a numpy restatement of DESIGN.md §9 rank 5 rules 1-7 that shares no code with it.

CPU only.  Each test prints its measured worst case; the bounds are the named constants below (10x a measured worst
difference of the reference's own route, or what the number format promises) and DESIGN.md §9 rank 5 holds the same
table."""
import ctypes as C
import math

import numpy as np

import pose_ref as P
from test_pose import (DP, K_ANISO, K_KITTI, aniso_cases, bad_point_cases, case_inputs, check_bad_points, gpu_cases,
                       grid_cases, grid_hits_the_chunk_edges, rot, scene, seq, seq_pose, skew)  # noqa: F401

SQRT_BOUND_ULP = 1.0  # six Newton steps from a guess within 6 %: the last step's rounding, no more
SOLVE5_WORST = 4.2e-8  # measured worst matched |E_ref - E_seq| (max norm, up to sign); numpy's eigenvalue route's error
SOLVE5_BOUND = 10 * SOLVE5_WORST
DECOMPOSE_WORST = 1.8e-15  # measured worst absolute difference of R1, R2, t from numpy's SVD
DECOMPOSE_BOUND = 10 * DECOMPOSE_WORST
RUN_RT_BOUND = 1e-12  # R and t of the whole run


def dp(a):
    return a.ctypes.data_as(DP)


def normalise(p, K=K_KITTI):
    p = np.asarray(p, np.float32)
    return (p[:, 0].astype(np.float64) - K[0, 2]) / K[0, 0], (p[:, 1].astype(np.float64) - K[1, 2]) / K[1, 1]


def solve5_seq(lib, x1, y1, x2, y2):
    pts = np.ascontiguousarray(np.r_[x1, y1, x2, y2], np.float64)
    out = np.zeros(90)
    n = lib.seq_solve5(dp(pts), dp(out))
    return out[:9 * n].reshape(n, 3, 3).copy()


def decompose_seq(lib, E):
    E = np.ascontiguousarray(E, np.float64).reshape(9)
    R1, R2, t = np.zeros(9), np.zeros(9), np.zeros(3)
    ok = lib.seq_decompose(dp(E), dp(R1), dp(R2), dp(t))
    return ok, R1.reshape(3, 3), R2.reshape(3, 3), t


def essential(rng, maxdeg):
    R = rot(rng, maxdeg)
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    E = skew(t) @ R
    return E / np.linalg.norm(E), R, t


# ---- 1. samples -----------------------------------------------------------------------------------------------------


def test_samples_equal_the_integer_restatement(seq):
    idx = (C.c_uint32 * 5)()
    for seed in (0, 5, 2**63 + 12345, 2**64 - 1):
        for n in (5, 6, 7, 100, 3000, 2**31):
            for it in range(200):
                ref = P.sample(seed, it, n)
                assert seq.seq_sample(seed, it, n, idx) == 1 and list(idx) == ref, (seed, n, it)
                assert len(set(ref)) == 5 and all(0 <= v < n for v in ref)
    hist = np.zeros(7)
    for it in range(20000):
        assert seq.seq_sample(5, it, 7, idx) == 1
        hist[list(idx)] += 1
    share = hist / hist.sum()
    print("sample shares at n = 7: %.4f-%.4f" % (share.min(), share.max()))
    assert np.abs(share - 1 / 7).max() <= 0.01
    # fewer than 5 points: the draws run out on both sides
    assert P.sample(1, 0, 4) is None and seq.seq_sample(1, 0, 4, idx) == 0


# ---- 2. RANSACUpdateNumIters ----------------------------------------------------------------------------------------


def near_half_integer(p, ep):
    q = P.niters_quotient(p, ep)
    if q is None or q[1] >= 0:
        return False
    return abs((q[0] / q[1]) % 1.0 - 0.5) <= 1e-9


def test_update_niters_equals_the_math_log_restatement(seq):
    total = left_out = 0
    for prob in (0.999, 0.99, 0.5, 0.0, 1.0):
        for n in (5, 20, 100, 939, 3000):
            for count in range(n + 1):
                ep = (n - count) / n
                for max_iters in (1000, 7, 1):
                    total += 1
                    if near_half_integer(prob, ep):
                        left_out += 1
                        continue
                    assert seq.seq_update_niters(prob, ep, max_iters) == P.update_niters(prob, ep, max_iters), \
                        (prob, n, count, max_iters)
    print("update_niters: %d triples, %d left out" % (total, left_out))
    assert total == 61035 and left_out <= total // 1000
    # prob and ep outside [0, 1] are clamped
    for max_iters in (1000, 7, 1):
        for ep in np.linspace(0.0, 1.0, 41):
            for prob, clamped in ((-1.0, 0.0), (-1e-300, 0.0), (1 + 1e-9, 1.0), (2.0, 1.0), (1e300, 1.0),
                                  (float("inf"), 1.0), (float("-inf"), 0.0)):
                ref = P.update_niters(clamped, ep, max_iters)
                assert P.update_niters(prob, ep, max_iters) == ref
                assert near_half_integer(clamped, ep) or seq.seq_update_niters(prob, ep, max_iters) == ref, (prob, ep)
        for prob in (0.999, 0.5):
            for ep, clamped in ((-0.5, 0.0), (-1e-12, 0.0), (-1e300, 0.0), (1 + 1e-7, 1.0), (2.0, 1.0), (1e10, 1.0)):
                ref = P.update_niters(prob, clamped, max_iters)
                assert P.update_niters(prob, ep, max_iters) == ref
                assert seq.seq_update_niters(prob, ep, max_iters) == ref, (prob, ep)


# ---- 3. pose_sqrt ---------------------------------------------------------------------------------------------------


def test_restated_sqrt_within_1_ulp(seq):
    rng = np.random.default_rng(11)
    xs = np.concatenate([rng.uniform(0, 4, 100_000), 10.0 ** rng.uniform(-320, 308, 100_000)])
    assert (xs < 2.2250738585072014e-308).sum() > 1000  # subnormals are in
    worst = 0.0
    for x in xs:
        ref = math.sqrt(x)
        got = seq.seq_sqrt(float(x))
        if got != ref:
            worst = max(worst, abs(got - ref) / math.ulp(ref))
    print("pose_sqrt worst %.2f ulp" % worst)
    assert worst <= SQRT_BOUND_ULP
    inf, nan = float("inf"), float("nan")
    assert seq.seq_sqrt(0.0) == 0.0 and seq.seq_sqrt(-0.0) == 0.0 and seq.seq_sqrt(-1.0) == 0.0
    assert seq.seq_sqrt(-inf) == 0.0 and seq.seq_sqrt(inf) == inf and math.isnan(seq.seq_sqrt(nan))
    for x in (5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, 1.0, 4.0):
        assert abs(seq.seq_sqrt(x) - math.sqrt(x)) <= math.ulp(math.sqrt(x)), x


# ---- 4. Sampson error -----------------------------------------------------------------------------------------------


def test_sampson_decisions_equal_the_matrix_restatement(seq):
    """Thresholds 0.5, 1 and 3 px.  Threshold 0 is in the whole-run test's grid, where it is compared like every
    other input."""
    models = flagged = pairs = 0
    s = 0
    while models < 200:
        outliers, noise, threshold = [0.0, 0.3, 0.6][s % 3], ["sigma", "round"][s % 2], [1.0, 0.5, 3.0][s % 4 % 3]
        p1, p2, *_ = scene(3000 + s, 1000, outliers, noise)
        (x1, y1), (x2, y2) = normalise(p1), normalise(p2)
        thr = threshold / K_KITTI[0, 0]
        tf = np.float32(thr * thr)
        idx = P.sample(s, 0, 1000)
        for E in solve5_seq(seq, x1[idx], y1[idx], x2[idx], y2[idx])[:200 - models]:
            err, e32 = P.sampson(E, x1, y1, x2, y2)
            got = np.array([seq.seq_sampson(dp(E), x1[p], y1[p], x2[p], y2[p]) for p in range(1000)], np.float32)
            f = P.sampson_flagged(err, tf)
            assert np.array_equal((got <= tf)[~f], (e32 <= tf)[~f]), (s, models)
            flagged += int(f.sum())
            pairs += 1000
            models += 1
        s += 1
    print("sampson: %d pairs, %d flagged" % (pairs, flagged))
    assert pairs == 200_000 and flagged <= pairs // 100_000


# ---- 5. the minimal solver, both ways -------------------------------------------------------------------------------


def nearest(E, models):
    if len(models) == 0:
        return np.inf
    return min(min(np.abs(E - M).max(), np.abs(E + M).max()) for M in models)


def solve5_problems():
    out = []
    for s in range(250):
        p1, p2, *_ = scene(9000 + s, 5)
        out.append(normalise(p1) + normalise(p2))
    rng = np.random.default_rng(5)
    for s in range(250):
        out.append(tuple(rng.uniform(-0.8, 0.8, (4, 5))))
    return out


def test_minimal_solver_is_complete_and_sound_against_the_action_matrix(seq):
    worst, roots, left_out, missed, extra = 0.0, 0, 0, 0, 0
    probs = solve5_problems()
    for k, (x1, y1, x2, y2) in enumerate(probs):
        ref, cond = P.solve5_ref(x1, y1, x2, y2)
        got = solve5_seq(seq, x1, y1, x2, y2)
        close = any(min(np.abs(ref[i] - ref[j]).max(), np.abs(ref[i] + ref[j]).max()) < 100 * SOLVE5_BOUND
                    for i in range(len(ref)) for j in range(i))
        if cond > 1e10 or close:
            left_out += 1
            continue
        roots += len(ref)
        d_ref = [nearest(E, got) for E in ref]
        d_got = [nearest(E, ref) for E in got]
        missed += sum(d > SOLVE5_BOUND for d in d_ref)
        extra += sum(d > SOLVE5_BOUND for d in d_got)
        worst = max([worst] + [d for d in d_ref + d_got if d <= max(SOLVE5_BOUND, 1e-5)])
    print("solve5: %d roots, worst matched difference %.3g, %d missed, %d extra, %d problems left out"
          % (roots, worst, missed, extra, left_out))
    assert missed == 0 and extra == 0
    assert worst <= SOLVE5_WORST * 1.25  # the recorded figure (and DESIGN's table) still is what this measures
    assert left_out <= len(probs) // 50 and roots > 1500


# ---- 6. decomposeEssentialMat ---------------------------------------------------------------------------------------


def test_decompose_equals_numpy_svd(seq):
    rng = np.random.default_rng(6)
    worst = 0.0
    for k in range(2000):
        E, R, t = essential(rng, 180.0)
        if k % 2:
            E = -E
        ok, R1, R2, tu = decompose_seq(seq, E)
        assert ok == 1
        r1, r2, u3 = P.decompose(E)
        d = min(max(np.abs(R1 - r1).max(), np.abs(R2 - r2).max()), max(np.abs(R1 - r2).max(), np.abs(R2 - r1).max()))
        d = max(d, min(np.abs(tu - u3).max(), np.abs(tu + u3).max()))
        d = max(d, min(np.abs(R1 - R).max(), np.abs(R2 - R).max()), min(np.abs(tu - t).max(), np.abs(tu + t).max()))
        for Q in (R1, R2):
            d = max(d, abs(np.linalg.det(Q) - 1.0), np.abs(Q.T @ Q - np.eye(3)).max())
        d = max(d, abs(np.linalg.norm(tu) - 1.0))
        worst = max(worst, d)
    print("decompose worst %.3g" % worst)
    assert worst <= DECOMPOSE_BOUND
    assert worst <= DECOMPOSE_WORST * 1.25  # the recorded figure (and DESIGN's table) still is what this measures
    R1, R2, tu = np.full(9, 7.0), np.full(9, 7.0), np.full(3, 7.0)
    assert seq.seq_decompose(dp(np.zeros(9)), dp(R1), dp(R2), dp(tu)) == 0 and P.decompose(np.zeros((3, 3))) is None


# ---- 7. the cheirality test -----------------------------------------------------------------------------------------


def test_point_good_equals_lstsq_depths(seq):
    """Scene 0 is scaled to depths of 30-70, so the first camera's depths lie on both sides of 50; scene 1 moves
    backwards through depths of 48-51, so that points with z1 < 50 < z2 exercise the second camera's bound."""
    points = flagged = good = beyond = beyond2 = behind = 0
    back = np.array([0.1, 0.05, 1.0]) / np.linalg.norm([0.1, 0.05, 1.0])
    for s in range(50):
        depth = [(30.0, 70.0), (48.0, 51.0)][s] if s < 2 else (2.0, 40.0)
        p1, p2, R, t, _ = scene(4000 + s, 100, 0.2, ["sigma", "round", "none"][s % 3], depth=depth,
                                t=back if s == 1 else None)
        (x1, y1), (x2, y2) = normalise(p1), normalise(p2)
        E = skew(t) @ R
        ok, R1, R2, tu = decompose_seq(seq, E / np.linalg.norm(E))
        assert ok == 1
        for Rc, sg in ((R1, 1.0), (R2, 1.0), (R1, -1.0), (R2, -1.0)):  # the winner and the three losers
            z1, z2 = P.depths(Rc, sg * tu, x1, y1, x2, y2)
            ref = P.depth_good(z1, z2)
            f = P.depth_flagged(z1, z2)
            Rc = np.ascontiguousarray(Rc)
            got = np.array([seq.seq_point_good(dp(Rc), dp(tu), sg, x1[p], y1[p], x2[p], y2[p]) for p in range(100)])
            assert np.array_equal(got[~f] != 0, ref[~f]), (s, sg)
            points += 100
            flagged += int(f.sum())
            good += int(ref.sum())
            if s == 0:
                beyond += int(((z1 > P.DIST_THRESH) & (z2 > 0)).sum())
            if s == 1:
                beyond2 += int(((z1 > 0) & (z1 < P.DIST_THRESH) & (z2 > P.DIST_THRESH)).sum())
            behind += int((z1 < 0).sum())
    print("point_good: %d points, %d good, %d with z1 > 50 in scene 0, %d with z1 < 50 < z2 in scene 1, %d behind, "
          "%d flagged" % (points, good, beyond, beyond2, behind, flagged))
    assert flagged <= points // 1000
    assert good > 3000 and behind > 3000 and beyond >= 20 and beyond2 >= 10  # every side of every bound is exercised


# ---- 8. the whole run -----------------------------------------------------------------------------------------------


def run_inputs():
    out = []
    for cs in gpu_cases():
        if cs["n"] <= 1000 or (cs["n"] == 3000 and not any(o[0] == "n3000" for o in out)):
            out.append(("n3000" if cs["n"] == 3000 else "gpu_cases", K_KITTI, None) + case_inputs(cs))
    grid = grid_cases()
    out += [("grid", K_KITTI, None) + case_inputs(cs) for cs in grid]
    out += [("aniso", K_ANISO, None, p1, p2, kw) for p1, p2, kw in aniso_cases()]
    out += [("bad", K_KITTI, (bad,), p1, p2, kw) for p1, p2, bad, kw in bad_point_cases()]
    return out, grid


def same_candidate(r, cand):
    R, t, good, mask = cand
    return (np.abs(r["R"] - R).max() <= RUN_RT_BOUND and np.abs(r["t"] - t).max() <= RUN_RT_BOUND and
            r["good"] == good and np.array_equal(r["mask"], mask))


def test_whole_run_equals_the_numpy_restatement(seq):
    inputs, grid = run_inputs()
    tied = 0
    worst = 0.0
    grid_iters = []
    for name, K, bad, p1, p2, kw in inputs:
        got = seq_pose(seq, p1, p2, K=K, **kw)
        ref = P.ref_pose(p1, p2, K, kw["prob"], kw["threshold"], kw["max_iters"], kw["seed"],
                         lambda *a: solve5_seq(seq, *a))
        what = (name, len(p1), kw)
        assert ref["flag_sampson"] == 0 and ref["flag_depth"] == 0, what  # every comparison below is decided
        assert (got["iters"], got["inliers"]) == (ref["iters"], ref["inliers"]), what
        assert np.array_equal(got["E"], ref["E"]), what
        if name == "grid":
            grid_iters.append(ref["iters"])
        if bad is not None:
            check_bad_points(ref, bad[0], len(p1), kw)
        if ref["inliers"] == 0:
            assert np.array_equal(got["R"], np.eye(3)) and not got["t"].any() and not got["mask"].any(), what
            assert got["good"] == 0
            continue
        top = max(ref["cand_good"])
        first = [c for c in ref["candidates"] if c[2] == top]
        if len(first) > 1:  # which tied candidate is "first" follows Jacobi's eigenvector signs: any of them
            tied += 1
            assert ref["inliers"] < 100, what
        assert any(same_candidate(got, c) for c in first), what
        c = [c for c in first if same_candidate(got, c)][0]
        worst = max(worst, np.abs(got["R"] - c[0]).max(), np.abs(got["t"] - c[1]).max())
    print("whole run: %d cases, %d tied, worst R / t difference %.3g" % (len(inputs), tied, worst))
    assert grid_hits_the_chunk_edges(grid_iters, grid), sorted(set(grid_iters))
    assert tied <= len(inputs) // 10
