"""Independent numpy restatement of the landmark building of tracked windows (the reference's
buildLandmarksFromFirstTwoFramesAndTracks, src/with_bundle_adjustment.cpp:502-575) and the synthetic scenes of
tests/test_landmarks_ref.py, tests/test_landmarks.py and tests/test_cpp_landmarks.py.

Nothing here shares code with the library: Rodrigues through math.sin / math.cos, the DLT through numpy.linalg.svd
of the 4 x 4 system itself (the library diagonalises its normal matrix with Jacobi sweeps)."""
import math

import numpy as np

# KITTI sequence 00 camera (tests/test_pose.py: K_KITTI)
K_KITTI = np.array([[718.856, 0.0, 607.1928], [0.0, 718.856, 185.2157], [0.0, 0.0, 1.0]])
IMG_W, IMG_H = 1241, 376
OK, BASELINE, EMPTY, BAD_POSE = range(4)


def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def rodrigues(v):
    v = np.asarray(v, float)
    th = float(np.linalg.norm(v))
    if th < 1e-12:
        return np.eye(3) + hat(v)
    k = hat(v / th)
    return np.eye(3) + math.sin(th) * k + (1.0 - math.cos(th)) * (k @ k)


def rotvec(R):
    """Angle-axis of a rotation matrix, angle in [0, pi) (through the unit quaternion)."""
    q = np.array([1.0 + R[0, 0] + R[1, 1] + R[2, 2], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    assert q[0] > 1e-3, "rotation too close to pi for this helper"
    q = q / np.linalg.norm(q)
    s = np.linalg.norm(q[1:])
    if s < 1e-300:
        return np.zeros(3)
    return q[1:] / s * (2.0 * math.atan2(s, q[0]))


def rot_x(deg):
    return rodrigues(np.array([math.radians(deg), 0.0, 0.0]))


# the world frame in which about a fifth of the points in front of both cameras has world z <= 0
WORLD_TILTED = (rot_x(-80.0), np.zeros(3))
WORLD_PLAIN = (np.eye(3), np.zeros(3))


def make_scene(seed, W=5, slots=200, sigma=0.0, outliers=0.0, world=WORLD_PLAIN, min_seen=0, depth_sign=1.0,
               pose_pert=0.0, step=None, K=K_KITTI):
    """One window.  W cameras along a gently turning path (steps of 0.5-1.5 units -- `step`: that length for the first
    one --, at most 3 degrees per step) seen from the world frame X_w = R X + t of `world`; `slots` points at depth
    6-40 of camera 0 (depth_sign = -1: behind it), slot s observed in frames 0 .. seen[s] - 1 with seen[s] uniform in
    [min_seen, W] and cut where the point comes closer than 0.5 to a camera.  sigma: pixel noise; outliers: share of
    the observations of frames >= 2 moved by 5-50 px; pose_pert: perturbation of the poses 2 .. handed out (rad and
    units; poses 0 and 1, which the landmarks are built from, stay true).  Pixels are float32, zero past `seen`, as
    the windows tracker leaves them.
    Returns poses (W, 6: angle-axis, translation, world -> camera), tracks (slots, W, 2) float32, seen (slots,)
    int32, X (slots, 3) the true world points, parallax (slots,) in degrees between the rays of cameras 0 and 1."""
    rng = np.random.default_rng(seed)
    Rg, tg = np.asarray(world[0], float), np.asarray(world[1], float)
    Rwc, c = [np.eye(3)], [np.zeros(3)]
    for i in range(W - 1):
        a = np.array([rng.uniform(-0.3, 0.3), 1.0, rng.uniform(-0.3, 0.3)])
        dR = rodrigues(a / np.linalg.norm(a) * math.radians(rng.uniform(-3.0, 3.0)))
        d = np.array([rng.uniform(-0.05, 0.05), rng.uniform(-0.02, 0.02), 1.0])
        length = rng.uniform(0.5, 1.5)
        if i == 0 and step is not None:
            length = step
        c.append(c[-1] + Rwc[-1] @ (d / np.linalg.norm(d) * length))
        Rwc.append(Rwc[-1] @ dR)
    Rwc = [Rg @ R for R in Rwc]
    c = [Rg @ x + tg for x in c]
    poses = np.array([np.r_[rotvec(R.T), -R.T @ x] for R, x in zip(Rwc, c)])
    pix = np.c_[rng.uniform(0, IMG_W, slots), rng.uniform(0, IMG_H, slots), np.ones(slots)]
    X = c[0] + (np.linalg.inv(K) @ pix.T).T * (depth_sign * rng.uniform(6.0, 40.0, slots))[:, None] @ Rwc[0].T
    seen = rng.integers(min_seen, W + 1, slots).astype(np.int32)
    tracks = np.zeros((slots, W, 2))
    for k in range(W):
        p = (X - c[k]) @ Rwc[k]  # rows: Rwc^T (X - c)
        near = depth_sign * p[:, 2] < 0.5
        seen = np.where(near & (seen > k), k, seen).astype(np.int32)
        z = np.where(near, 1.0, p[:, 2])
        tracks[:, k, 0] = K[0, 0] * p[:, 0] / z + K[0, 2]
        tracks[:, k, 1] = K[1, 1] * p[:, 1] / z + K[1, 2]
    if sigma > 0:
        tracks = tracks + rng.normal(0.0, sigma, tracks.shape)
    if outliers > 0 and W > 2:
        bad = rng.random((slots, W)) < outliers
        bad[:, :2] = False
        ang = rng.uniform(0, 2 * math.pi, (slots, W))
        r = rng.uniform(5.0, 50.0, (slots, W))
        tracks = tracks + bad[..., None] * np.stack([r * np.cos(ang), r * np.sin(ang)], axis=-1)
    live = np.arange(W)[None, :] < seen[:, None]
    tracks = np.where(live[..., None], tracks, 0.0).astype(np.float32)
    r0, r1 = X - c[0], X - c[1]
    cosang = np.sum(r0 * r1, axis=1) / (np.linalg.norm(r0, axis=1) * np.linalg.norm(r1, axis=1))
    parallax = np.degrees(np.arccos(np.clip(cosang, -1.0, 1.0)))
    poses_out = poses.copy()
    for i in range(2, W):
        if pose_pert > 0:
            a = rng.normal(size=3)
            R = rodrigues(a / np.linalg.norm(a) * pose_pert) @ rodrigues(poses[i, :3])
            poses_out[i] = np.r_[rotvec(R), poses[i, 3:] + rng.normal(0.0, 5.0 * pose_pert, 3)]
    return dict(poses=poses_out, true_poses=poses, tracks=tracks, seen=seen, X=X, parallax=parallax)


def stack(scenes):
    """Scenes of one slot count and window length as a batch: poses (n, W, 6), tracks (n, slots, W, 2), seen (n, slots)."""
    return (np.stack([s["poses"] for s in scenes]), np.stack([s["tracks"] for s in scenes]),
            np.stack([s["seen"] for s in scenes]))


def np_dlt(P0, P1, x0, x1):
    """cv::triangulatePoints' linear system of one correspondence, solved by numpy's SVD: the homogeneous point."""
    A = np.array([x0[0] * P0[2] - P0[0], x0[1] * P0[2] - P0[1], x1[0] * P1[2] - P1[0], x1[1] * P1[2] - P1[1]])
    return np.linalg.svd(A)[2][-1]


def np_build(K, poses, tracks, seen):
    """One window by the rules of DESIGN.md §9 rank 10 in numpy: (status, points (N, 3), slot_of_point (N,),
    obs_point (M,), obs_pose (M,), obs_xy (M, 2))."""
    poses = np.asarray(poses, float).reshape(-1, 6)
    W = len(poses)
    empty = (np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2)))
    if any(np.linalg.norm(p[:3]) > 1e5 for p in poses[:2]):
        return (BAD_POSE,) + empty
    b = float(np.linalg.norm(poses[0, 3:] - poses[1, 3:]))
    if b < 0.1 or b > 100.0:
        return (BASELINE,) + empty
    P = [K @ np.c_[rodrigues(p[:3]), p[3:]] for p in poses[:2]]
    pts, slot, op, oq, xy = [], [], [], [], []
    for s in range(len(seen)):
        n = int(min(max(seen[s], 0), W))
        if n < 2:
            continue
        t = np.asarray(tracks[s], np.float64)
        h = np_dlt(P[0], P[1], t[0], t[1])
        if h[3] == 0.0:
            continue
        with np.errstate(all="ignore"):
            X = h[:3] / h[3]
        if not np.all(np.isfinite(X)) or not X[2] > 0.0:
            continue
        for k in range(n):
            op.append(len(pts)), oq.append(k), xy.append(t[k])
        pts.append(X), slot.append(s)
    if not pts:
        return (EMPTY,) + empty
    return OK, np.array(pts), np.array(slot, np.int32), np.array(op, np.int32), np.array(oq, np.int32), np.array(xy)
