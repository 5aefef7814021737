"""Independent numpy restatement of the join of overlapping windows into one trajectory (the
reference's src/with_bundle_adjustment.cpp:203 and :234-249), the generator of the streams of
tests/test_stitch_ref.py and tests/test_stitch.py, and the tolerance of both.

Nothing here shares code with the library: rel(w, k) is inverse(P(w, 0)) @ P(w, k) with numpy.linalg.inv (a
Gauss-Jordan inverse in numpy.longdouble, window_poses_ref.inverse) and numpy's matrix product, the baselines come
from numpy.sqrt, and the fold multiplies whole 4x4 matrices -- the library inverts in closed form and sums every dot
product left to right.  Every function takes a dtype, so that the tolerance can be measured.

The tolerance.  TOLERANCE_REL is 16 x the largest distance between this restatement in float64 and in longdouble over
cases(), each distance (the largest absolute difference over trajectory, anchors and lambda) divided by the case's
scale(): the largest absolute translation entry among the window poses, T_start and the trajectory, at least 1.  The
margin is the one tests/window_poses_ref.py gives its TOLERANCE: two correctly rounded routes may differ by more than
one run shows.  A comparison on a case holds when its distance is at most tolerance(case) = TOLERANCE_REL x scale().
Measured by tests/test_stitch_ref.py (which asserts that what it measures is not above the value here): the largest
scaled distance is 2.06e-15 (case W130_L8_s6_scaled: 1.04e-12 at a scale of 505), over cases() with scales from 5 to
870 units; 16 x that, rounded up, is the value below.  On the same cases the library is within 2.3e-15 x scale of the
longdouble route and within 4.6e-15 x scale of the true path (the longdouble route itself: 5.7e-15, the rounding of
the inputs to float64).
"""
import numpy as np

import window_poses_ref as WR

OK, BROKEN, SCALE_UNALIGNED = 0, 1, 2
SHAPES = ((1, 2, 1), (2, 3, 1), (7, 2, 1), (5, 5, 2), (65, 5, 3), (130, 8, 7), (130, 8, 6))  # (W, L, stride)

TOLERANCE_REL = 16 * 2.1e-15


def frames(W, L, stride):
    return (W - 1) * stride + L


def owner_table(W, L, stride):
    """rule 1: (owner (F,), index in the window (F,))"""
    f = np.arange(frames(W, L, stride))
    w = np.minimum(W - 1, f // stride)
    return w.astype(np.int32), (f - w * stride).astype(np.int32)


def _similar(M, s, dtype):
    """the rigid M with its translation multiplied by s"""
    out = np.array(M, dtype)
    out[:3, 3] = dtype(s) * out[:3, 3]
    out[3] = np.array([0, 0, 0, 1], dtype)
    return out


def stitch(poses, stride, T_start=None, align_scale=False, dtype=np.float64):
    """poses (W, L, 4, 4) -> dict of trajectory4x4 (F, 4, 4), owner (F,), anchors4x4 (W, 4, 4), lambda (W,), status
    (W,) by the rules of DESIGN.md §9 rank 16, in `dtype`."""
    raw = np.asarray(poses, np.float64)
    W, L = raw.shape[:2]
    P = np.array(raw, dtype)
    one = dtype(1)
    broken = [not np.isfinite(raw[w]).all() for w in range(W)]
    rel, b_first, b_link = [], [], []
    for w in range(W):
        if broken[w]:
            rel.append([np.eye(4, dtype=dtype)] * L)
            b_first.append(dtype(0)), b_link.append(dtype(0))
            continue
        inv0 = WR.inverse(P[w, 0], dtype)
        rel.append([inv0 @ P[w, k] for k in range(L)])
        c = P[w, :, :3, 3]
        dist = lambda a, b: np.sqrt(np.sum((c[b] - c[a]) ** 2))
        b_first.append(dist(0, 1))
        b_link.append(dist(stride, stride + 1) if stride <= L - 2 else dtype(0))
    G = np.eye(4, dtype=dtype) if T_start is None else np.array(T_start, dtype).reshape(4, 4)
    Lam = one
    anchors, lams, status = [], [], []
    usable = lambda b: bool(np.isfinite(np.float64(b))) and b > 0
    for w in range(W):
        st = OK
        if broken[w]:
            st = BROKEN
        elif w > 0 and align_scale:
            q = b_link[w - 1] / b_first[w] if usable(b_link[w - 1]) and usable(b_first[w]) else dtype(0)
            if usable(q):
                Lam = Lam * q
            else:
                st = SCALE_UNALIGNED
        anchors.append(G), lams.append(Lam), status.append(st)
        G = G @ _similar(rel[w][stride], Lam, dtype)
    own, idx = owner_table(W, L, stride)
    traj = [anchors[w] @ _similar(rel[w][k], lams[w], dtype) for w, k in zip(own, idx)]
    return {"trajectory4x4": np.array(traj), "owner": own, "anchors4x4": np.array(anchors), "lambda": np.array(lams),
            "status": np.array(status, np.int32)}


def distance(a, b):
    """the largest absolute difference over trajectory, anchors and lambda of two results (in longdouble)"""
    ld = np.longdouble
    return float(max(np.max(np.abs(np.asarray(a[k], ld) - np.asarray(b[k], ld)))
                     for k in ("trajectory4x4", "anchors4x4", "lambda")))


def scale(case, result):
    """the largest absolute translation entry among the case's window poses, T_start and the result's trajectory, at
    least 1"""
    t = [np.abs(np.asarray(case["poses"], np.float64)[..., :3, 3]).max(),
         np.abs(np.asarray(result["trajectory4x4"], np.float64)[..., :3, 3]).max()]
    if case["T_start"] is not None:
        t.append(np.abs(np.asarray(case["T_start"], np.float64)[:3, 3]).max())
    return float(max(1.0, *t))


def tolerance(case, result):
    return TOLERANCE_REL * scale(case, result)


# ---- the streams of the tests ------------------------------------------------------------------------------------

def true_path(F, seed, dtype=np.longdouble):
    """F camera -> world poses along a gently turning path: steps of 0.5-1.5 units, at most 3 degrees per step,
    starting from a pose that is not the identity"""
    rng = np.random.default_rng(seed)
    T = np.array(WR.rigid(WR.rot(rng.normal(size=3), 0.7), rng.normal(size=3) * 3.0), dtype)
    out = [T]
    for _ in range(F - 1):
        a = np.array([rng.uniform(-0.3, 0.3), 1.0, rng.uniform(-0.3, 0.3)])
        dR = WR.exp_map(a / np.linalg.norm(a) * np.radians(rng.uniform(-3.0, 3.0)), dtype)
        d = np.array([rng.uniform(-0.05, 0.05), rng.uniform(-0.02, 0.02), 1.0])
        step = np.eye(4, dtype=dtype)
        step[:3, :3] = dR
        step[:3, 3] = np.array(d / np.linalg.norm(d) * rng.uniform(0.5, 1.5), dtype)
        T = T @ step
        out.append(T)
    return np.array(out)


def make_stream(W, L, stride, seed, scaled):
    """A true trajectory of F poses cut into W windows of L frames, window w from frame w * stride, each put into a
    gauge of its own: a rigid motion that takes the window's first camera to a random pose near the origin (rotation
    of up to 1 rad, translation of a few units: a window comes out of its chain in a local frame, its first pose the
    identity, and this keeps the rounding of the inputs to float64 as small as it is there) and, from window 1 on
    and when `scaled`, a scale in [0.3, 3] about its first camera.  Built in longdouble and rounded to float64
    once.  Returns dict of poses (W, L, 4, 4) float64, T_start (4, 4) float64 = the true pose of frame 0, true
    (F, 4, 4) longdouble = the true path from the ROUNDED T_start, gauge_scale (W,)."""
    ld = np.longdouble
    rng = np.random.default_rng(seed + 7919)
    path = true_path(frames(W, L, stride), seed)
    T_start = np.array(path[0], np.float64)
    # the path the stitch can recover starts at the T_start it is given: move the true path onto the rounded one
    shift = np.array(T_start, ld) @ WR.inverse(path[0], ld)
    path = np.array([shift @ T for T in path])
    poses, scales = np.zeros((W, L, 4, 4)), np.ones(W)
    for w in range(W):
        win = path[w * stride:w * stride + L]
        s = rng.uniform(0.3, 3.0) if scaled and w > 0 else 1.0
        B = np.array(WR.rigid(WR.rot(rng.normal(size=3), rng.uniform(0.0, 1.0)), rng.normal(size=3) * 3.0), ld)
        A = B @ WR.inverse(win[0], ld)
        for k in range(L):
            T = np.array(win[k], ld)
            T[:3, 3] = win[0][:3, 3] + ld(s) * (win[k][:3, 3] - win[0][:3, 3])
            poses[w, k] = np.array(A @ T, np.float64)
        scales[w] = s
    return dict(poses=poses, T_start=T_start, true=path, gauge_scale=scales, stride=stride, scaled=scaled,
                name="W%d_L%d_s%d_%s" % (W, L, stride, "scaled" if scaled else "rigid"))


_cases = None


def cases():
    """every shape of SHAPES with rigid gauges (align_scale off) and, where rule 3 allows it (stride <= L - 2), with
    scale gauges (align_scale on); each dict also carries align_scale"""
    global _cases
    if _cases is None:
        _cases = []
        for i, (W, L, stride) in enumerate(SHAPES):
            for scaled in (False, True):
                if scaled and stride > L - 2:
                    continue
                cs = make_stream(W, L, stride, 100 + i, scaled)
                cs["align_scale"] = scaled
                _cases.append(cs)
    return _cases


# ---- a stream of tracked windows over one scene (the stream-entry tests on the GPU) -------------------------------

def scene_stream(W, L, stride, slots, seed, K=None):
    """One camera path of F frames through one 3-D scene, geometry as landmarks_ref.make_scene's (steps of 0.5-1.5
    units, at most 3 degrees per step, points at depth 6-40): window w tracks `slots` points of its own, drawn in the
    image of its first camera, through its L frames -- slot s observed in frames 0 .. seen[s] - 1, cut where the point
    comes closer than 0.5 to a camera; no noise.  Returns dict of tracks (W, slots, L, 2) float32, seen (W, slots)
    int32, true (F, 4, 4) float64 camera -> world, K."""
    import landmarks_ref as LR

    K = LR.K_KITTI if K is None else K
    rng = np.random.default_rng(seed)
    path = np.array(true_path(frames(W, L, stride), seed, np.float64), np.float64)
    tracks, seen = np.zeros((W, slots, L, 2)), np.full((W, slots), L, np.int32)
    Kinv = np.linalg.inv(K)
    for w in range(W):
        cams = path[w * stride:w * stride + L]
        pix = np.c_[rng.uniform(0, LR.IMG_W, slots), rng.uniform(0, LR.IMG_H, slots), np.ones(slots)]
        X = cams[0][:3, 3] + ((Kinv @ pix.T).T * rng.uniform(6.0, 40.0, slots)[:, None]) @ cams[0][:3, :3].T
        for k in range(L):
            p = (X - cams[k][:3, 3]) @ cams[k][:3, :3]  # rows: R^T (X - c)
            near = p[:, 2] < 0.5
            seen[w] = np.where(near & (seen[w] > k), k, seen[w])
            z = np.where(near, 1.0, p[:, 2])
            tracks[w, :, k, 0] = K[0, 0] * p[:, 0] / z + K[0, 2]
            tracks[w, :, k, 1] = K[1, 1] * p[:, 1] / z + K[1, 2]
        tracks[w][np.arange(L)[None, :] >= seen[w][:, None]] = 0.0  # zero past `seen`, as the tracker leaves them
    return dict(tracks=tracks.astype(np.float32), seen=seen, true=path, K=K)


def similarity_residual(trajectory, true):
    """the largest distance between the camera centres of `trajectory` and of `true` after the one similarity
    (Umeyama: scale, rotation, translation) that fits the first onto the second best, and the largest rotation
    angle between the orientations after that rotation: (units, rad)"""
    A = np.asarray(trajectory, np.float64)[:, :3, 3]
    B = np.asarray(true, np.float64)[:, :3, 3]
    ma, mb = A.mean(axis=0), B.mean(axis=0)
    U, D, Vt = np.linalg.svd((B - mb).T @ (A - ma) / len(A))
    S = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    Rs = U @ S @ Vt
    s = np.trace(np.diag(D) @ S) / ((A - ma) ** 2).sum(axis=1).mean()
    fit = s * (A - ma) @ Rs.T + mb
    ang = 0.0
    for Ta, Tb in zip(np.asarray(trajectory, np.float64), np.asarray(true, np.float64)):
        c = (np.trace((Rs @ Ta[:3, :3]).T @ Tb[:3, :3]) - 1.0) / 2.0
        ang = max(ang, float(np.arccos(np.clip(c, -1.0, 1.0))))
    return float(np.linalg.norm(fit - B, axis=1).max()), ang
