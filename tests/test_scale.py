"""Triangulation, relative scale and trajectory chaining (the reference's get_scale and pose chaining, DESIGN.md §9
rank 6).

CPU: the sequential restatement (tests/cpp/scale_sequential.cpp) against numpy and known answers on synthetic
three-frame scenes, and the host-only chaining entry.  GPU: the kernels against that restatement, bit for bit, and
the batched path against the host-array entries."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from test_pose import K_KITTI, NFEAT, H, W, kitti_batch, rot, seq_pose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = C.POINTER(C.c_double)
CXX = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC"]
SEEDS = range(24)
NOISES = ("none", "sigma", "round")


@pytest.fixture(scope="module")
def seq(tmp_path_factory):
    """The sequential restatement, compiled here (test infrastructure; not part of build())."""
    out = tmp_path_factory.mktemp("scale_seq") / "scale_sequential.so"
    subprocess.check_call(CXX + ["-o", str(out), os.path.join(ROOT, "tests", "cpp", "scale_sequential.cpp")])
    lib = C.CDLL(str(out))
    lib.seq_triangulate_homogeneous.argtypes = [C.c_void_p, C.c_void_p, C.c_int, DP, DP, DP, C.c_void_p]
    lib.seq_triangulate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, DP, DP, DP, C.c_void_p, C.c_void_p]
    lib.seq_estimate_scale.restype = C.c_double
    lib.seq_estimate_scale.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                       C.POINTER(C.c_int)]
    lib.seq_join_scale.restype = C.c_double
    lib.seq_join_scale.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, DP, DP, C.c_void_p, C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int),
                                   C.POINTER(C.c_int)]
    return lib


@pytest.fixture(scope="module")
def pose_seq(tmp_path_factory):
    """The relative-pose restatement of tests/test_pose.py, for the scenes whose poses are estimated."""
    out = tmp_path_factory.mktemp("scale_pose_seq") / "pose_sequential.so"
    subprocess.check_call(CXX + ["-o", str(out), os.path.join(ROOT, "tests", "cpp", "pose_sequential.cpp")])
    lib = C.CDLL(str(out))
    lib.seq_estimate_pose.argtypes = [C.c_void_p, C.c_void_p, C.c_int, DP, C.c_double, C.c_double, C.c_int,
                                      C.c_uint64] + [C.c_void_p] * 7
    return lib


def _d(a):
    a = np.ascontiguousarray(a, np.float64)
    return a, a.ctypes.data_as(DP)


def _pts(p):
    return np.ascontiguousarray(np.asarray(p, np.float32).reshape(-1, 2))


def _p(a):
    return None if a is None else a.ctypes.data


def seq_triangulate(lib, p1, p2, R, t, K=K_KITTI):
    p1, p2 = _pts(p1), _pts(p2)
    n = len(p1)
    (K, kp), (R, rp), (t, tp) = _d(K), _d(R), _d(t)
    xyz = np.zeros((max(n, 1), 3), np.float32)
    valid = np.zeros(max(n, 1), np.uint8)
    lib.seq_triangulate(p1.ctypes.data, p2.ctypes.data, n, kp, rp, tp, xyz.ctypes.data, valid.ctypes.data)
    return xyz[:n], valid[:n]


def seq_homogeneous(lib, p1, p2, R, t, K=K_KITTI):
    p1, p2 = _pts(p1), _pts(p2)
    n = len(p1)
    (K, kp), (R, rp), (t, tp) = _d(K), _d(R), _d(t)
    h = np.zeros((max(n, 1), 4))
    lib.seq_triangulate_homogeneous(p1.ctypes.data, p2.ctypes.data, n, kp, rp, tp, h.ctypes.data)
    return h[:n]


def _xyz(a):
    return np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, 3))


def _valid(v):
    return None if v is None else np.ascontiguousarray(np.asarray(v).reshape(-1) != 0, np.uint8)


def seq_scale(lib, prev, cur, pv=None, cv=None):
    prev, cur, pv, cv = _xyz(prev), _xyz(cur), _valid(pv), _valid(cv)
    used = C.c_int(0)
    s = lib.seq_estimate_scale(prev.ctypes.data, _p(pv), len(prev), cur.ctypes.data, _p(cv), len(cur), C.byref(used))
    return s, used.value


def seq_join(lib, t12, xyz12, valid12, R12, t12v, q23, xyz23, valid23):
    """-> scale, triplets as (position in the 1 -> 2 list, position in the 2 -> 3 list), ratios used"""
    t12 = np.ascontiguousarray(t12, np.int32)
    q23 = np.ascontiguousarray(q23, np.int32)
    xyz12, xyz23, valid12, valid23 = _xyz(xyz12), _xyz(xyz23), _valid(valid12), _valid(valid23)
    (R12, rp), (t12v, tp) = _d(R12), _d(t12v)
    ti = np.zeros(max(len(q23), 1), np.int32)
    tj = np.zeros(max(len(q23), 1), np.int32)
    nt, used = C.c_int(0), C.c_int(0)
    s = lib.seq_join_scale(t12.ctypes.data, len(t12), xyz12.ctypes.data, _p(valid12), rp, tp,
                           q23.ctypes.data, len(q23), xyz23.ctypes.data, _p(valid23), ti.ctypes.data, tj.ctypes.data,
                           C.byref(nt), C.byref(used))
    return s, list(zip(ti[:nt.value].tolist(), tj[:nt.value].tolist())), used.value


def scene3(seed, n, noise="sigma", outliers=0.0, depth=(6.0, 40.0), maxdeg=3.0, K=K_KITTI):
    """A static scene seen from three poses, x2 = R12 x1 + t12 (|t12| = 1), x3 = R23 x2 + t23 with |t23| / |t12| drawn
    from [0.5, 2]; the keypoints of frame 2 are numbered by a random permutation of the points.  Returns the match
    lists of both pairs in query order, as the matcher would: (query index, train index, pts of the query frame,
    pts of the train frame), the true poses (unit t) and the step ratio."""
    rng = np.random.default_rng(seed)
    R12, R23 = rot(rng, maxdeg), rot(rng, maxdeg)
    ratio = rng.uniform(0.5, 2.0)

    def step():
        t = np.array([rng.normal(0, 0.2), rng.normal(0, 0.1), -1.0])
        return t / np.linalg.norm(t)

    t12, u23 = step(), step()
    t23 = ratio * u23
    Ki = np.linalg.inv(K)
    pix = [np.zeros((0, 2))] * 3
    while len(pix[0]) < n:
        m = 2 * n + 16
        px = np.c_[rng.uniform(0, W, m), rng.uniform(0, H, m), np.ones(m)]
        X1 = (Ki @ px.T).T * rng.uniform(*depth, (m, 1))
        X2 = (R12 @ X1.T).T + t12
        X3 = (R23 @ X2.T).T + t23
        ok = (X2[:, 2] > 0.5) & (X3[:, 2] > 0.5)
        q2 = (K @ (X2[ok] / X2[ok, 2:]).T).T
        q3 = (K @ (X3[ok] / X3[ok, 2:]).T).T
        ins = np.ones(len(q2), bool)
        for q in (q2, q3):
            ins &= (q[:, 0] > -50) & (q[:, 0] < W + 50) & (q[:, 1] > -50) & (q[:, 1] < H + 50)
        pix = [np.r_[pix[0], px[ok][ins, :2]], np.r_[pix[1], q2[ins, :2]], np.r_[pix[2], q3[ins, :2]]]
    p1, p2, p3 = (p[:n].copy() for p in pix)
    if noise == "sigma":
        p1, p2, p3 = (p + rng.normal(0, 0.3, p.shape) for p in (p1, p2, p3))
    elif noise == "round":
        p1, p2, p3 = np.round(p1), np.round(p2), np.round(p3)
    # a wrong match: the train point of the pair is anywhere in the image
    p2a, p3a = p2.copy(), p3.copy()
    o12, o23 = rng.random(n) < outliers, rng.random(n) < outliers
    p2a[o12] = np.c_[rng.uniform(0, W, o12.sum()), rng.uniform(0, H, o12.sum())]
    p3a[o23] = np.c_[rng.uniform(0, W, o23.sum()), rng.uniform(0, H, o23.sum())]
    idx2 = rng.permutation(n)  # frame-2 keypoint index of point i
    inv2 = np.argsort(idx2)  # point of frame-2 keypoint j
    f32 = np.float32
    pair12 = (np.arange(n, dtype=np.int32), idx2.astype(np.int32), p1.astype(f32), p2a.astype(f32))
    pair23 = (np.arange(n, dtype=np.int32), inv2.astype(np.int32), p2[inv2].astype(f32), p3a[inv2].astype(f32))
    return dict(pair12=pair12, pair23=pair23, R12=R12, t12=t12, R23=R23, t23=u23, ratio=ratio)


def scene_scale(lib, sc, poses=None):
    """rules 1, 2, 4, 3 on a scene3 through the restatement; poses: ((R12, t12), (R23, t23)), default: the truth"""
    (R12, t12), (R23, t23) = poses or ((sc["R12"], sc["t12"]), (sc["R23"], sc["t23"]))
    _, tr12, a1, a2 = sc["pair12"]
    q23, _, b2, b3 = sc["pair23"]
    x12, v12 = seq_triangulate(lib, a1, a2, R12, t12)
    x23, v23 = seq_triangulate(lib, b2, b3, R23, t23)
    return seq_join(lib, tr12, x12, v12, R12, t12, q23, x23, v23)


# ---- CPU: the arithmetic against numpy ----------------------------------------------


def svd_points(p1, p2, R, t, K=K_KITTI):
    """rule 1's A per point, solved by numpy.linalg.svd: the Euclidean points in double"""
    P1 = K @ np.c_[np.eye(3), np.zeros(3)]
    P2 = K @ np.c_[R, t]
    out = np.zeros((len(p1), 3))
    for i, (a, b) in enumerate(zip(_pts(p1).astype(np.float64), _pts(p2).astype(np.float64))):
        A = np.stack([a[0] * P1[2] - P1[0], a[1] * P1[2] - P1[1], b[0] * P2[2] - P2[0], b[1] * P2[2] - P2[1]])
        h = np.linalg.svd(A)[2][3]
        out[i] = h[:3] / h[3]
    return out


# measured over the 72 scenes below (seeds 0-23 x 3 noise kinds, both pairs, 300 points each): 5.29e-12
TRI_SVD_MEASURED = 5.3e-12
TRI_SVD_BOUND = 100 * TRI_SVD_MEASURED


def test_triangulation_against_numpy_svd(seq):
    worst = 0.0
    for noise in NOISES:
        for s in SEEDS:
            sc = scene3(s, 300, noise)
            for pair, R, t in (("pair12", sc["R12"], sc["t12"]), ("pair23", sc["R23"], sc["t23"])):
                _, _, a, b = sc[pair]
                h = seq_homogeneous(seq, a, b, R, t)
                got = h[:, :3] / h[:, 3:]
                ref = svd_points(a, b, R, t)
                rel = np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)
                worst = max(worst, rel.max())
                xyz, valid = seq_triangulate(seq, a, b, R, t)
                assert valid.all() and np.array_equal(xyz, got.astype(np.float32))  # rule 2
    print("triangulation vs numpy.linalg.svd: worst relative difference %.3g (bound %.3g)" % (worst, TRI_SVD_BOUND))
    assert worst <= TRI_SVD_BOUND


def scale_errors(seq, noise, poses_of=None, outliers=0.0):
    errs = []
    for s in SEEDS:
        sc = scene3(s, 300, noise, outliers)
        scale, trip, used = scene_scale(seq, sc, poses_of(sc) if poses_of else None)
        assert len(trip) == 300 and used <= 299
        errs.append(abs(scale - sc["ratio"]) / sc["ratio"])
    return np.array(errs)


# largest relative error of the rule-4 scale against |t23| / |t12| over seeds 0-23, as measured
# (DESIGN.md §9 rank 6); the tests bound it at 10x (noiseless) and 2x (the others) of these
SCALE_ERR_NOISELESS = 4.5e-7  # 4.44e-07, median 1.4e-07: the float Point3f
SCALE_ERR_SIGMA = 0.0126  # 1.25 %, median 0.44 %
SCALE_ERR_ROUND = 0.0130  # 1.29 %, median 0.45 %
SCALE_ERR_ESTIMATED_POSE = 0.0955  # 9.54 %, median 3.3 %: poses from the restatement, 30 % wrong matches per pair


def test_scale_of_noiseless_scenes(seq):
    e = scale_errors(seq, "none")
    print("noiseless: worst %.3g median %.3g" % (e.max(), np.median(e)))
    assert e.max() <= 10 * SCALE_ERR_NOISELESS


@pytest.mark.parametrize("noise,measured", [("sigma", "SCALE_ERR_SIGMA"), ("round", "SCALE_ERR_ROUND")])
def test_scale_of_noisy_scenes(seq, noise, measured):
    e = scale_errors(seq, noise)
    print("%s: worst %.3g median %.3g" % (noise, e.max(), np.median(e)))
    assert e.max() <= 2 * globals()[measured]


def test_scale_with_estimated_poses_and_outliers(seq, pose_seq):
    """Both poses from the relative-pose restatement on match lists with 30 % wrong matches each (sigma = 0.3 px)."""

    def poses_of(sc):
        out = []
        for pair in ("pair12", "pair23"):
            _, _, a, b = sc[pair]
            r = seq_pose(pose_seq, a, b)
            out.append((r["R"], r["t"]))
        return out

    e = scale_errors(seq, "sigma", poses_of, outliers=0.3)
    print("estimated poses, 30 %% outliers: worst %.3g median %.3g" % (e.max(), np.median(e)))
    assert e.max() <= 2 * SCALE_ERR_ESTIMATED_POSE


def np_scale(prev, cur, pv=None, cv=None):
    """rule 3 in explicit float32 numpy: products summed left to right, np.sqrt on float32, the upper median"""
    prev, cur = _xyz(prev), _xyz(cur)
    if len(prev) == 0 or len(cur) == 0:
        return 1.0, 0
    with np.errstate(over="ignore", invalid="ignore"):
        return _np_scale(prev, cur, pv, cv)


def _np_scale(prev, cur, pv, cv):
    m = min(len(prev), len(cur))
    pv = np.ones(len(prev), bool) if pv is None else np.asarray(pv, bool)
    cv = np.ones(len(cur), bool) if cv is None else np.asarray(cv, bool)

    def dist(a, b):
        d = a - b
        assert d.dtype == np.float32
        s = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        assert type(s) is np.float32
        return np.sqrt(s)

    ratios = []
    for i in range(1, m):
        if pv[i] and pv[i - 1] and cv[i] and cv[i - 1]:
            r = float(dist(prev[i], prev[i - 1])) / (float(dist(cur[i], cur[i - 1])) + 1e-6)
            if math.isfinite(r):  # distances that overflow a float: no ratio
                ratios.append(r)
    if not ratios:
        return 1.0, 0
    return max(0.1, min(5.0, sorted(ratios)[len(ratios) // 2])), len(ratios)


def scale_cases():
    """(prev, cur, prev_valid, cur_valid) lists for rule 3: even and odd ratio counts, both clamps, unequal lengths,
    lists of 0, 1 and 2 points, an invalid point in each of the four positions"""
    rng = np.random.default_rng(5)
    cases = []
    for n in (0, 1, 2, 3, 4, 5, 6, 64, 65, 300, 301):
        a = rng.normal(0, 10, (n, 3)).astype(np.float32)
        cases.append((a, (a / np.float32(1.7) + rng.normal(0, 0.05, (n, 3))).astype(np.float32), None, None))
    a = rng.normal(0, 10, (50, 3)).astype(np.float32)
    cases.append((a, a * np.float32(100), None, None))  # clamp at 0.1
    cases.append((a, a * np.float32(0.01), None, None))  # clamp at 5
    cases.append((a, np.repeat(a[:1], 50, 0), None, None))  # cur distances 0: the 1e-6 of the denominator
    b = rng.normal(0, 10, (37, 3)).astype(np.float32)
    cases += [(a, b, None, None), (b, a, None, None), (a, b[:0], None, None), (a[:0], b, None, None),
              (a[:1], b, None, None), (a, b[:2], None, None)]
    for k in (0, 1, 17, 36):  # an invalid point at the first, second, an inner and the last aligned index
        pv, cv = np.ones(50, np.uint8), np.ones(37, np.uint8)
        pv[k] = 0
        cases.append((a, b, pv, None))
        cases.append((a, b, None, 1 - (np.arange(37) == k)))
        cases.append((a, b, pv, 1 - (np.arange(37) == (k + 1) % 37)))
    cases.append((a, b, np.zeros(50, np.uint8), None))  # no ratio at all
    cases.append((a[:2], b[:2], np.array([1, 0]), None))
    # finite points so far apart that dx * dx overflows a float: inf / inf (NaN) and inf / finite are no ratios
    far = a.copy()
    far[7, 0] = np.float32(3e19)
    cases += [(far, far, None, None), (far, a, None, None), (a, far, None, None), (far[6:9], far[6:9], None, None)]
    return cases


def test_rule3_bit_equal_to_float32_numpy(seq):
    counts = set()
    for prev, cur, pv, cv in scale_cases():
        got = seq_scale(seq, prev, cur, pv, cv)
        ref = np_scale(prev, cur, pv, cv)
        assert got == ref, (len(prev), len(cur))
        assert 0.1 <= got[0] <= 5.0
        counts.add(ref[1] % 2 if ref[1] else None)
    assert counts == {None, 0, 1}
    # the upper median of an even count: 4 ratios 1, 2, 3, 4 (in another order) -> 3, not numpy's 2.5
    cur = np.cumsum(np.ones((5, 3), np.float32), 0) / np.float32(math.sqrt(3))
    prev = np.zeros((5, 3), np.float32)
    prev[1:, 0] = np.cumsum([3, 1, 4, 2])
    s, used = seq_scale(seq, prev, cur)
    assert used == 4 and abs(s - 3) < 1e-4
    assert seq_scale(seq, prev * 10, cur) == (5.0, 4) and seq_scale(seq, prev / 100, cur) == (0.1, 4)


def py_join(t12, q23):
    """src/feature_tracking_scale.py:127-164's dictionaries, iterated in ascending frame-2 index"""
    m12 = {}
    for i, m in enumerate(t12):
        m12[int(m)] = i  # the last write in query order wins
    m23 = {int(q): j for j, q in enumerate(q23)}
    return [(m12[k], m23[k]) for k in sorted(set(m12) & set(m23))]


def test_rule4_join_on_hand_built_match_tables(seq):
    rng = np.random.default_rng(9)
    R, t = np.eye(3), np.zeros(3)

    def run(q12, t12, q23):
        x12 = rng.normal(0, 5, (len(q12), 3)).astype(np.float32)
        x23 = rng.normal(0, 5, (len(q23), 3)).astype(np.float32)
        s, trip, used = seq_join(seq, t12, x12, None, R, t, q23, x23, None)
        assert trip == py_join(t12, q23)
        # rule 3 on the joined lists (R = I, t = 0: the transform is exact)
        assert (s, used) == seq_scale(seq, x12[[i for i, _ in trip]], x23[[j for _, j in trip]])
        return s, trip, used

    # duplicate train indices: queries 1, 4 and 6 all matched frame-2 keypoint 7 -> the largest query (position 3)
    s, trip, used = run([0, 1, 4, 6, 9], [3, 7, 7, 7, 5], [2, 3, 5, 7, 8])
    assert trip == [(0, 1), (4, 2), (3, 3)] and used == 2
    # unmatched queries on either side
    s, trip, used = run([0, 2, 5, 8], [10, 4, 6, 1], [1, 2, 3, 4, 11])
    assert trip == [(3, 0), (1, 3)] and used == 1
    # an empty intersection, empty lists
    assert run([0, 1], [4, 5], [6, 7]) == (1.0, [], 0)
    assert run([], [], [1, 2]) == (1.0, [], 0)
    assert run([1, 2], [3, 4], []) == (1.0, [], 0)
    # one triplet: no consecutive pair
    assert run([0, 1], [4, 5], [5, 9]) == (1.0, [(1, 0)], 0)
    # random tables with many duplicates
    for s in range(20):
        r = np.random.default_rng(100 + s)
        n12, n23 = int(r.integers(1, 200)), int(r.integers(1, 150))
        q12 = np.sort(r.choice(400, n12, replace=False))
        t12 = r.integers(0, 120, n12)
        q23 = np.sort(r.choice(150, n23, replace=False))
        run(q12, t12, q23)


def test_rule4_moves_the_previous_points_into_the_shared_frame(seq):
    """X' = R X + t in double from the float point, cast back to float; an invalid point drops its two ratios."""
    sc = scene3(3, 40, "none")
    _, t12, a1, a2 = sc["pair12"]
    q23, _, b2, b3 = sc["pair23"]
    x12, v12 = seq_triangulate(seq, a1, a2, sc["R12"], sc["t12"])
    x23, v23 = seq_triangulate(seq, b2, b3, sc["R23"], sc["t23"])
    s, trip, used = seq_join(seq, t12, x12, v12, sc["R12"], sc["t12"], q23, x23, v23)
    moved = (x12.astype(np.float64) @ sc["R12"].T + sc["t12"]).astype(np.float32)
    ref = np_scale(moved[[i for i, _ in trip]], x23[[j for _, j in trip]])
    assert used == 39 and abs(s - ref[0]) <= 1e-6 * ref[0]  # numpy's matmul may sum in another order
    v = v12.copy()
    v[trip[5][0]] = 0
    assert seq_join(seq, t12, x12, v, sc["R12"], sc["t12"], q23, x23, v23)[2] == 37


def random_poses(rng, n):
    T = [np.eye(4)]
    T[0][:3, :3] = rot(rng, 180)
    T[0][:3, 3] = rng.normal(0, 10, 3)
    for _ in range(n):
        S = np.eye(4)
        S[:3, :3] = rot(rng, 5)
        d = rng.normal(size=3)
        S[:3, 3] = d / np.linalg.norm(d) * rng.uniform(0.5, 2.0)
        T.append(T[-1] @ S)
    return np.array(T)


def test_chain_trajectory(pkg):
    rng = np.random.default_rng(1)
    poses = random_poses(rng, 999)  # 1000 poses
    R, t, s = [], [], []
    for a, b in zip(poses[:-1], poses[1:]):
        T = np.linalg.inv(b) @ a  # cur = prev T^-1
        R.append(T[:3, :3])
        s.append(np.linalg.norm(T[:3, 3]))
        t.append(T[:3, 3] / s[-1])
    got = pkg.chain_trajectory(poses[0], R, t, s)
    assert got.shape == poses.shape and np.array_equal(got[0], poses[0])
    extent = np.ptp(poses[:, :3, 3], axis=0).max()
    err = np.abs(got - poses).max()
    print("chaining 999 steps: worst deviation %.3g of an extent of %.3g" % (err, extent))
    assert err <= 1e-9 * extent
    # the reference's own arithmetic, with a general inverse
    cur = poses[0].copy()
    for i in range(5):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R[i], s[i] * t[i]
        cur = cur @ np.linalg.inv(T)
        assert np.abs(cur - got[i + 1]).max() <= 1e-12 * extent
    only = pkg.chain_trajectory(poses[3], np.zeros((0, 3, 3)), np.zeros((0, 3)), np.zeros(0))
    assert only.shape == (1, 4, 4) and np.array_equal(only[0], poses[3])
    # ones as scales: unit steps along the same directions
    unit = pkg.chain_trajectory(poses[0], R[:10], t[:10], np.ones(10))
    steps = np.linalg.norm(np.diff(unit[:, :3, 3], axis=0), axis=1)
    assert np.abs(steps - 1).max() <= 1e-12


# ---- GPU ---------------------------------------------------------------------------------


def gpu_scale_cases():
    cases = []
    ns = [0, 1, 2, 5, 63, 64, 65, 300, 1000, 3000]
    for i in range(30):
        cases.append(dict(seed=i, n=ns[i % len(ns)], outliers=[0.0, 0.2, 0.5, 0.8][i % 4],
                          noise=["sigma", "round"][(i // 2) % 2], drop=[0, 0, 3][i % 3]))
    return cases


@pytest.mark.gpu
def test_gpu_triangulate_and_estimate_scale_equal_sequential(pkg, seq):
    with pkg.Context(pkg.default_params("gpu")) as c:

        def check(a1, a2, R12, t12, b2, b3, R23, t23, drop=0, what=None):
            lists = []
            for p, q, R, t in ((a1, a2, R12, t12), (b2, b3, R23, t23)):
                xyz, valid = c.triangulate(p, q, K_KITTI, R, t)
                rx, rv = seq_triangulate(seq, p, q, R, t)
                assert xyz.dtype == np.float32 and xyz.tobytes() == rx.tobytes(), what
                assert np.array_equal(valid, rv), what
                lists.append((xyz, valid))
            (x12, v12), (x23, v23) = lists
            x12, v12 = x12[:len(x12) - drop], v12[:len(v12) - drop]  # n_prev != n_cur
            for pv, cv in ((v12, v23), (None, None), (v12, None)):
                assert c.estimate_scale(x12, x23, pv, cv) == seq_scale(seq, x12, x23, pv, cv), what
            return lists

        for cs in gpu_scale_cases():
            sc = scene3(cs["seed"], max(cs["n"], 1), cs["noise"], cs["outliers"])
            n = cs["n"]
            (_, _, a1, a2), (_, _, b2, b3) = sc["pair12"], sc["pair23"]
            check(a1[:n], a2[:n], sc["R12"], sc["t12"], b2[:n], b3[:n], sc["R23"], sc["t23"], min(cs["drop"], n), cs)
        for prev, cur, pv, cv in scale_cases():  # rule 3's own list, with the overflowing distances
            assert c.estimate_scale(prev, cur, pv, cv) == seq_scale(seq, prev, cur, pv, cv), (len(prev), len(cur))
        # the degenerate ones
        sc = scene3(77, 200)
        (_, _, a1, a2), (_, _, b2, b3) = sc["pair12"], sc["pair23"]
        I, z = np.eye(3), np.zeros(3)
        # identical point pairs under a real pose, and under rank 5's degenerate pose (R = I, t = 0: P2 = P1)
        check(a1, a1, sc["R12"], sc["t12"], b2, b2, sc["R23"], sc["t23"], what="identical pairs")
        got = check(a1, a2, I, z, b2, b3, I, z, what="t = 0, R = I")
        check(a1, a1, I, z, np.repeat(b2[:1], 200, 0), np.repeat(b2[:1], 200, 0), I, z, what="identical, degenerate")
        pp = np.repeat(np.array([[K_KITTI[0, 2], K_KITTI[1, 2]]], np.float32), 70, 0)
        check(pp, pp, sc["R12"], sc["t12"], pp, a2[:70], I, z, what="principal point")
        print("t = 0, R = I: %d of %d points valid" % (got[0][1].sum(), len(got[0][1])))


def batched_scale(pkg, c, frames, K, w=W, h=H):
    """batch -> match -> pose -> scale; returns everything the checks need"""
    cap = c.plan(w, h)["out_capacity"]
    c.batch_host(frames)
    c.batch_match_consecutive(0.8)
    kps = c.batch_fetch(0, len(frames), cap)["kps"]
    matches = [c.batch_match_fetch(pair, cap)[:2] for pair in range(len(frames) - 1)]
    c.batch_pose_consecutive(K)
    poses = c.batch_pose_fetch()
    c.batch_scale_consecutive(K)
    res = c.batch_scale_fetch()
    points = [c.batch_points_fetch(pair) for pair in range(len(frames) - 1)]
    return dict(kps=kps, matches=matches, poses=poses, scale=res, points=points)


def check_batched_against_host_entries(c, seq, b, K):
    npairs = len(b["matches"])
    assert len(b["scale"]["scale"]) == npairs
    for pair in range(npairs):
        qi, ti = b["matches"][pair]
        xyz, valid = b["points"][pair]
        assert len(xyz) == len(qi) == len(valid)
        p1, p2 = b["kps"][pair][qi].astype(np.float32), b["kps"][pair + 1][ti].astype(np.float32)
        R, t = b["poses"]["R"][pair], b["poses"]["t"][pair]
        hx, hv = c.triangulate(p1, p2, K, R, t)
        assert xyz.tobytes() == hx.tobytes() and np.array_equal(valid, hv), pair
        sx, sv = seq_triangulate(seq, p1, p2, R, t, K)
        assert xyz.tobytes() == sx.tobytes() and np.array_equal(valid, sv), pair
        got = (b["scale"]["scale"][pair], int(b["scale"]["triplets"][pair]), int(b["scale"]["ratios_used"][pair]))
        if pair == 0:
            assert got == (1.0, 0, 0)
            continue
        q0, t0 = b["matches"][pair - 1]
        x0, v0 = b["points"][pair - 1]
        s, trip, used = seq_join(seq, t0, x0, v0, b["poses"]["R"][pair - 1], b["poses"]["t"][pair - 1], qi, xyz, valid)
        assert got == (s, len(trip), used), (pair, got, s, len(trip), used)
        assert 0.1 <= got[0] <= 5.0


@pytest.mark.gpu
def test_gpu_batched_scale_equals_host_array_entries(pkg, seq, pose_seq):
    k0, k1 = O.load_kitti(0), O.load_kitti(1)
    frames = np.stack([k0, k1, k0, k1, k0])
    p = pkg.default_params("gpu", nfeatures=NFEAT, max_width=W, max_height=H, max_batch=8)
    with pkg.Context(p) as c:
        b = batched_scale(pkg, c, frames, K_KITTI)
        check_batched_against_host_entries(c, seq, b, K_KITTI)
    sc = b["scale"]
    # the same frames at another position of the batch give the same bits
    assert b["points"][0][0].tobytes() == b["points"][2][0].tobytes()
    assert np.array_equal(b["points"][0][1], b["points"][2][1])
    assert (sc["scale"][1], sc["triplets"][1], sc["ratios_used"][1]) == (sc["scale"][3], sc["triplets"][3], sc["ratios_used"][3])
    print("scales", sc["scale"], "triplets", sc["triplets"], "ratios", sc["ratios_used"],
          "valid", [int(v.sum()) for _, v in b["points"]], "of", [len(v) for _, v in b["points"]])
    # k0 -> k1 -> k0: the true step ratio is 1.  How far a single seed's estimate is from it is bounded by what
    # the restatement shows over the RANSAC seeds 0-39 on the same match lists, with a 2x margin (a single
    # seed's t scatters by about 7 degrees on this short-baseline pair).  Measured: scale
    # 1.061; over the seeds |log scale| 0.158 in the median, 1.22 at worst
    (q0, t0), (q1, t1) = b["matches"][0], b["matches"][1]
    kps = b["kps"]
    a1, a2 = kps[0][q0].astype(np.float32), kps[1][t0].astype(np.float32)
    b2, b3 = kps[1][q1].astype(np.float32), kps[2][t1].astype(np.float32)
    dev = []
    for s in range(40):
        r12, r23 = seq_pose(pose_seq, a1, a2, seed=s), seq_pose(pose_seq, b2, b3, seed=s)
        x12, v12 = seq_triangulate(seq, a1, a2, r12["R"], r12["t"])
        x23, v23 = seq_triangulate(seq, b2, b3, r23["R"], r23["t"])
        dev.append(abs(math.log(seq_join(seq, t0, x12, v12, r12["R"], r12["t"], q1, x23, v23)[0])))
    got = abs(math.log(sc["scale"][1]))
    print("k0 -> k1 -> k0: scale %.4f (|log| %.3f); over seeds 0-39 |log scale| median %.3f, worst %.3f"
          % (sc["scale"][1], got, np.median(dev), max(dev)))
    assert got == dev[0]  # seed 0 is the batched entry's default seed
    # on this pair 2 * max(dev) = 2.44 is above what the clamp to [0.1, 5] allows (ln 10): only the line above bites
    assert got <= 2 * max(dev)


@pytest.mark.gpu
def test_gpu_batched_scale_1080p_4000_features(pkg, seq):
    """The join's LDS (16 bytes per result slot) at the 1080p / 4000-feature configuration."""
    w, h = 1920, 1080
    K = np.array([[1000.0, 0, 960.0], [0, 1000.0, 540.0], [0, 0, 1]])
    # stream_b frames are independent of each other: one of them and a copy moved by (+5, +2) px, alternating, so
    # that consecutive frames match and most of pair 0's train keypoints are pair 1's queries
    f0 = pkg.streams.stream_b(1, h, w)[0]
    f1 = np.roll(f0, (2, 5), (0, 1))
    frames = np.stack([f0, f1, f0, f1])
    p = pkg.default_params("gpu", nfeatures=4000, nlevels=12, scale_factor=1.2, blur_levels=2, blur_kind=0, max_width=w,
                           max_height=h, max_batch=4)
    with pkg.Context(p) as c:
        assert c.plan(w, h)["out_capacity"] >= 4000
        b = batched_scale(pkg, c, frames, K, w, h)
        check_batched_against_host_entries(c, seq, b, K)
    print("1080p: matches", [len(q) for q, _ in b["matches"]], "scales", b["scale"]["scale"], "triplets",
          b["scale"]["triplets"], "ratios", b["scale"]["ratios_used"])
    # the join has real work at this size (measured: DESIGN.md §9 rank 6)
    assert (b["scale"]["triplets"][1:] > 1).all()


@pytest.mark.gpu
def test_gpu_scale_states_and_lanes(pkg):
    k0, k1 = O.load_kitti(0), O.load_kitti(1)
    frames = np.stack([k0, k1, k0])
    p = pkg.default_params("gpu", nfeatures=NFEAT, max_width=W, max_height=H, max_batch=4)
    with pkg.Context(p) as c:
        ref = batched_scale(pkg, c, frames, K_KITTI)
    with pkg.Context(p) as c:
        with pytest.raises(pkg.OrbxError) as e:
            c.batch_scale_fetch(0, 1)  # nothing scaled yet
        assert e.value.status == pkg.orbx.ERR_INVALID_ARG
        with pytest.raises(pkg.OrbxError):
            c.batch_points_fetch(0)
        kitti_batch(pkg, c, frames)
        with pytest.raises(pkg.OrbxError) as e:
            c.batch_scale_consecutive(K_KITTI)  # matched, not posed
        assert e.value.status == pkg.orbx.ERR_INVALID_ARG
        c.set_pipelined_batches(True)
        c.batch_host(np.stack([k1, k0, k1, k1]))  # another batch first, on the other lane
        c.batch_match_consecutive(0.8)
        c.batch_pose_consecutive(K_KITTI)
        got = batched_scale(pkg, c, frames, K_KITTI)
        for k in ref["scale"]:
            assert np.array_equal(got["scale"][k], ref["scale"][k]), k
        for (gx, gv), (rx, rv) in zip(got["points"], ref["points"]):
            assert gx.tobytes() == rx.tobytes() and np.array_equal(gv, rv)
        # fetches outside the last scaled batch
        for first, n in ((0, 3), (2, 1), (-1, 1)):
            with pytest.raises(pkg.OrbxError) as e:
                c.batch_scale_fetch(first, n)
            assert e.value.status == pkg.orbx.ERR_INVALID_ARG
        for pair in (-1, 2):
            with pytest.raises(pkg.OrbxError) as e:
                c.batch_points_fetch(pair)
            assert e.value.status == pkg.orbx.ERR_INVALID_ARG
        # capacity too small: the count comes back
        n0 = len(ref["points"][0][0])
        xyz, valid, cnt = np.zeros((n0, 3), np.float32), np.zeros(n0, np.uint8), C.c_int(0)
        st = pkg.orbx.load().orbx_batch_points_fetch(c._h, 0, xyz.ctypes.data_as(C.c_void_p),
                                                     valid.ctypes.data_as(C.c_void_p), n0 - 1, C.byref(cnt))
        assert st == pkg.orbx.ERR_CAPACITY and cnt.value == n0
        # the match table rewritten since the pose: by a host-array matcher call (it reuses the scratch) ...
        kitti_batch(pkg, c, frames)
        c.batch_pose_consecutive(K_KITTI)
        desc = np.random.default_rng(0).integers(0, 256, (40, 32), dtype=np.uint8)
        c.match_ratio(desc, desc[::-1].copy())
        with pytest.raises(pkg.OrbxError) as e:
            c.batch_scale_consecutive(K_KITTI)
        assert e.value.status == pkg.orbx.ERR_INVALID_ARG
        # ... or by another batch match: its matches are not the ones the poses came from
        kitti_batch(pkg, c, frames)
        c.batch_pose_consecutive(K_KITTI)
        c.batch_match_consecutive(0.7)
        with pytest.raises(pkg.OrbxError) as e:
            c.batch_scale_consecutive(K_KITTI)
        assert e.value.status == pkg.orbx.ERR_INVALID_ARG
        c.batch_pose_consecutive(K_KITTI)
        c.batch_scale_consecutive(K_KITTI)  # posed again on the new matches: accepted
        kitti_batch(pkg, c, frames)
        c.batch_pose_consecutive(K_KITTI)
        c.batch_scale_consecutive(K_KITTI)  # the reference state again, for the fetch below
        # another batch enqueued since the pose
        c.batch_host(frames)
        with pytest.raises(pkg.OrbxError) as e:
            c.batch_scale_consecutive(K_KITTI)
        assert e.value.status == pkg.orbx.ERR_INVALID_ARG
        # the last scaled batch can still be fetched
        assert np.array_equal(c.batch_scale_fetch(0, 2)["scale"], ref["scale"]["scale"])


CPP_MIRROR = r"""
#include "orb.hpp"
#include <cstdio>
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb");
  int n = 0;
  if (fread(&n, 4, 1, f) != 1) return 2;
  std::vector<float> raw((size_t)8 * n);
  if (fread(raw.data(), 4, raw.size(), f) != raw.size()) return 2;
  double Rt[24];
  if (fread(Rt, 8, 24, f) != 24) return 2;
  fclose(f);
  std::vector<orbx::Point2f> a1((size_t)n), a2((size_t)n), b2((size_t)n), b3((size_t)n);
  for (int i = 0; i < n; i++) {
    a1[i].x = raw[8 * i], a1[i].y = raw[8 * i + 1], a2[i].x = raw[8 * i + 2], a2[i].y = raw[8 * i + 3];
    b2[i].x = raw[8 * i + 4], b2[i].y = raw[8 * i + 5], b3[i].x = raw[8 * i + 6], b3[i].y = raw[8 * i + 7];
  }
  const double K[9] = {718.856, 0, 607.1928, 0, 718.856, 185.2157, 0, 0, 1};
  orbx::VisualOdomState vo;
  std::vector<orbx::Point3f> points_3d;
  const double s1 = orbx::get_scale(Rt, Rt + 9, a1, a2, K, points_3d, vo);
  vo.shift(points_3d);  // prev_points_3d = points_3d, src/feature_matching.cpp:87
  const double s2 = orbx::get_scale(Rt + 12, Rt + 21, b2, b3, K, points_3d, vo);
  printf("%a\n%a\n", s1, s2);
  for (int i = 0; i < 16; i++) vo.cur_pose[i] = (i % 5 == 0) ? 1.0 : 0.0;
  orbx::chain_pose(vo.cur_pose, Rt, Rt + 9, s1);
  orbx::chain_pose(vo.cur_pose, Rt + 12, Rt + 21, s2);
  for (double v : vo.cur_pose) printf("%a\n", v);
  return 0;
}
"""


@pytest.mark.gpu
def test_gpu_cpp_mirror_get_scale(pkg, tmp_path):
    src = tmp_path / "get_scale.cpp"
    src.write_text(CPP_MIRROR)
    exe = tmp_path / "get_scale.bin"
    pk = os.path.join(ROOT, "visual-odometry-gpu_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(pk, "host"), "-o", str(exe), str(src),
                           "-L" + pk, "-lorbx", "-Wl,-rpath," + pk, "-Wl,-rpath,/opt/rocm/lib"])
    sc = scene3(11, 300)
    (_, _, a1, a2), (_, _, b2, b3) = sc["pair12"], sc["pair23"]
    blob = tmp_path / "pts.bin"
    Rt = np.r_[sc["R12"].ravel(), sc["t12"], sc["R23"].ravel(), sc["t23"]].astype(np.float64)
    blob.write_bytes(np.int32(len(a1)).tobytes() + np.c_[a1, a2, b2, b3].astype(np.float32).tobytes() + Rt.tobytes())
    r = subprocess.run([str(exe), str(blob)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    vals = np.array([float.fromhex(v) for v in r.stdout.split()])
    with pkg.Context(pkg.default_params("gpu")) as c:
        x12, v12 = c.triangulate(a1, a2, K_KITTI, sc["R12"], sc["t12"])
        x23, v23 = c.triangulate(b2, b3, K_KITTI, sc["R23"], sc["t23"])
        s2, _ = c.estimate_scale(x12, x23, v12, v23)
    # the reference's C++ flavours align the two lists by bare index (the first call has no previous points)
    assert vals[0] == 1.0 and vals[1] == s2
    ref = pkg.chain_trajectory(np.eye(4), [sc["R12"], sc["R23"]], [sc["t12"], sc["t23"]], [1.0, s2])
    assert np.array_equal(vals[2:].reshape(4, 4), ref[2])
