"""The blocks of matcher, pose, scale, bundle adjustment and the pair tracker are reused and nobody notices (GPU).

Each of these context parts owns a few blocks whose sections csrc/orbx_layout.h places (MatchBlock, MatchInput,
PoseBlock, ScaleBlock, TriHost, ScaleHost, BaStage, LmWork, LkIo), grown on demand by ensure().  Here every path is
called small, large, small on ONE context: the small arrays end inside a 256-byte section, the large ones cross one
256-thread pass and make every block grow, and the second small call runs in blocks that hold the large call's stale
bytes.  Every result has to be bit-equal to the same call on a fresh context: a kernel or a copy that read beyond its
section, or wrote into its neighbour's, would show.  That is a consistency condition; correctness against the
references stays with the parity tests of each path (RANSAC is seeded, bundle adjustment is deterministic).
"""
import numpy as np
import pytest

import oracle_lib as O
from test_ba import K_KITTI, make_window

pytestmark = pytest.mark.gpu

W, H = 96, 64
K = np.array([[100.0, 0.0, 48.0], [0.0, 100.0, 32.0], [0.0, 0.0, 1.0]])
PATHS = ("matcher", "batch_chain", "estimate_pose", "triangulate_scale", "bundle_adjust", "lk_track")


def flat(x):
    """a result as nested lists of (dtype, shape, bytes): equal lists are bit-equal results"""
    if isinstance(x, dict):
        return [(k, flat(x[k])) for k in sorted(x)]
    if isinstance(x, (list, tuple)):
        return [flat(a) for a in x]
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, float):
        return np.float64(x).tobytes()
    return x


def context(pkg):
    return pkg.Context(pkg.default_params("gpu", nfeatures=400, nlevels=2, threshold=5, max_width=W, max_height=H,
                                          max_batch=6))


# ---- inputs: made once, left alone ----
def descriptors(nq, nt, seed):
    """nq queries and nt trains; the first trains are queries with a few bits flipped, so the ratio test passes some"""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    m = min(nq, nt) * 2 // 3
    t[:m] = q[:m] ^ (rng.integers(0, 256, (m, 32), dtype=np.uint8) & rng.integers(0, 256, (m, 32), dtype=np.uint8) & 0x11)
    return q, t


def crop():
    return np.ascontiguousarray(O.load_kitti(0)[300:300 + H, 480:480 + W])


def frames_of(n):
    """n frames of 96 x 64, each the one before moved by (1, 2).  Two frames: a 36 x 24 window of the crop on a flat
    frame (few keypoints); six: the whole crop"""
    img = crop()
    if n == 2:
        few = np.full_like(img, 89)
        few[20:44, 30:66] = img[20:44, 30:66]
        img = few
    return np.stack([np.roll(img, (k, 2 * k), axis=(0, 1)) for k in range(n)])


def correspondences(n, seed):
    """n points in front of two cameras a small motion apart, a fifth of them moved off their epipolar lines"""
    rng = np.random.default_rng(seed)
    X = np.c_[rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4, 12, n)]
    a = 0.03
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    t = np.array([0.3, 0.02, 0.1])
    p1 = X / X[:, 2:] @ K.T
    Y = X @ R.T + t
    p2 = Y / Y[:, 2:] @ K.T
    p2[::5, :2] += rng.uniform(3, 9, (len(p2[::5]), 2))
    return np.float32(p1[:, :2]), np.float32(p2[:, :2]), R, t / np.linalg.norm(t)


def ba_windows(n, W_, N, seed):
    ws = [make_window(seed + k, W_, N, sigma=0.3) for k in range(n)]
    return [(w["poses0"], w["pts0"], w["obs_point"], w["obs_pose"], w["obs_xy"]) for w in ws]


def lk_case(w, h, n, seed):
    """three images of w x h (a crop of kitti_000000 moved by (1, 2) per image) and n points inside them"""
    img = np.ascontiguousarray(O.load_kitti(0)[150:150 + h, 500:500 + w])
    rng = np.random.default_rng(seed)
    pts = np.float32(np.c_[rng.uniform(8, w - 8, n), rng.uniform(8, h - 8, n)])
    return [np.roll(img, (k, 2 * k), axis=(0, 1)) for k in range(3)], pts


# ---- one call of each path: everything the path gives back ----
def run_matcher(pkg, c, i, status=None):
    q, t = MATCHER[i]
    return (c.knn2(q, t), c.match_ratio(q, t, 0.8))


def run_batch_chain(pkg, c, i, status=None):
    """detect -> match -> pose -> scale with every fetch; then a host-array matcher call takes the match table, and
    the scale step has to refuse as it did before the two entries' results lay in one block"""
    frames = FRAMES[i]
    n = len(frames)
    cap = c.plan(W, H)["out_capacity"]
    assert cap >= 300
    c.batch_host(frames)
    c.batch_match_consecutive(0.8)
    c.batch_pose_consecutive(K, prob=0.999, threshold=1.0, max_iters=200, seed=7)
    c.batch_scale_consecutive(K)
    res = c.batch_fetch(0, n, cap)
    counts = res["counts"]
    out = dict(counts=counts, poses=c.batch_pose_fetch(), scales=c.batch_scale_fetch(),
               frames=[{k: res[k][f, :counts[f]].copy() for k in ("kps", "kps_level", "angles", "levels", "desc")}
                       for f in range(n)],
               matches=[c.batch_match_fetch(p, cap) for p in range(n - 1)],
               masks=[c.batch_pose_mask(p) for p in range(n - 1)],
               points=[c.batch_points_fetch(p) for p in range(n - 1)])
    if status is not None:
        status.append(dict(counts=counts.tolist(), matches=[len(m[0]) for m in out["matches"]],
                           inliers=out["poses"]["inliers"].tolist()))
    q, t = MATCHER[0]
    out["knn2_after"] = c.knn2(q, t)
    with pytest.raises(pkg.OrbxError) as e:
        c.batch_scale_consecutive(K)
    assert e.value.status == pkg.orbx.ERR_INVALID_ARG
    assert "the match table has been rewritten since the batch was posed" in str(e.value)
    return out


def run_estimate_pose(pkg, c, i, status=None):
    p1, p2, _, _ = POSE[i]
    r = c.estimate_pose(p1, p2, K, max_iters=200, seed=11)
    if status is not None:
        status.append((len(p1), r["inliers"], r["good"]))
    return r


def run_triangulate_scale(pkg, c, i, status=None):
    """orbx_estimate_scale directly after orbx_triangulate: the two lay out ONE buffer in turn"""
    p1, p2, R, t = TRI[i]
    xyz, valid = c.triangulate(p1, p2, K, R, t)
    xyz, valid = xyz.copy(), valid.copy()
    cur = np.float32(xyz * np.linspace(0.4, 0.6, len(xyz))[:, None])
    pv, cv = valid.copy(), valid.copy()
    pv[1::7], cv[2::5] = 0, 0  # (the valid bytes of both lists lie side by side in one section)
    scale = c.estimate_scale(xyz, cur, pv, cv)
    if status is not None:
        status.append((len(p1), int(valid.sum()), scale))
    return (xyz, valid, scale)


def run_bundle_adjust(pkg, c, i, status=None):
    got = c.bundle_adjust_batch(K_KITTI, BA[i], max_iters=10)
    if status is not None:
        status.append([g[2]["termination"] for g in got])
    return [(p.copy(), x.copy(), s) for p, x, s in got]


def run_lk_track(pkg, c, i, status=None):
    (a, b, d), pts = LK[i]
    first = c.lk_track(a, b, pts)
    then = c.lk_track(None, d, first[0])  # the continuation: b is the previous image
    if status is not None:
        status.append((len(pts), int(first[1].sum()), int(then[1].sum())))
    return (first, then)


MATCHER = [descriptors(5, 7, 1), descriptors(700, 900, 2), descriptors(5, 7, 1)]
FRAMES = [None] * 3
POSE = [correspondences(n, 20 + n) for n in (0, 8, 600, 8)]
TRI = [correspondences(n, 40 + n) for n in (4, 600, 4)]
BA = [None] * 3
LK = [None] * 3
RUN = dict(matcher=run_matcher, batch_chain=run_batch_chain, estimate_pose=run_estimate_pose,
           triangulate_scale=run_triangulate_scale, bundle_adjust=run_bundle_adjust, lk_track=run_lk_track)
CALLS = dict(matcher=3, batch_chain=3, estimate_pose=4, triangulate_scale=3, bundle_adjust=3, lk_track=3)


@pytest.fixture(scope="module")
def inputs():
    """the inputs that need the test image or a generated window: made once"""
    FRAMES[:] = [frames_of(2), frames_of(6), frames_of(2)]
    BA[:] = [ba_windows(1, 2, 6, 700), ba_windows(5, 4, 300, 710), ba_windows(1, 2, 6, 700)]
    LK[:] = [lk_case(64, 48, 5, 3), lk_case(192, 128, 300, 4), lk_case(64, 48, 5, 3)]


@pytest.fixture(scope="module")
def fresh(pkg, inputs):
    """every call of every path on a context of its own: what the one context has to reproduce"""
    out, status = {}, {}
    for path in PATHS:
        out[path], status[path] = [], []
        for i in range(CALLS[path]):
            with context(pkg) as c:
                out[path].append(flat(RUN[path](pkg, c, i, status[path])))
    return out, status


@pytest.fixture(scope="module")
def reused(pkg, inputs, fresh):
    """the same calls on ONE context, path after path"""
    with context(pkg) as c:
        return {path: [flat(RUN[path](pkg, c, i)) for i in range(CALLS[path])] for path in PATHS}


def test_the_shapes_exercise_the_paths(fresh):
    """not a comparison of nothing with nothing"""
    _, status = fresh
    print(status)
    small, large, _ = status["batch_chain"]
    assert 1 <= min(small["counts"]) and max(small["counts"]) < 256 < min(large["counts"])  # one 256-thread pass
    assert min(large["matches"]) >= 8 and min(large["inliers"]) >= 5
    assert [s[0] for s in status["estimate_pose"]] == [0, 8, 600, 8]
    assert status["estimate_pose"][0][1:] == (0, 0) and status["estimate_pose"][2][1] >= 300
    assert [s[0] for s in status["triangulate_scale"]] == [4, 600, 4]
    assert all(2 * s[1] >= s[0] for s in status["triangulate_scale"])
    assert status["triangulate_scale"][1][2][1] >= 100  # ratios entered the median
    assert [len(s) for s in status["bundle_adjust"]] == [1, 5, 1]
    assert [s[0] for s in status["lk_track"]] == [5, 300, 5] and status["lk_track"][1][2] >= 30


@pytest.mark.parametrize("path", PATHS)
def test_reused_blocks_equal_a_fresh_context(reused, fresh, path):
    for i in range(CALLS[path]):
        assert reused[path][i] == fresh[0][path][i], (path, i)
    if path != "estimate_pose":
        assert reused[path][0] == reused[path][2], path  # small, large, small: the large call left nothing behind
