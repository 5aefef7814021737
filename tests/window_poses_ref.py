"""Independent numpy restatement of the window-pose chain and the write-back gate (the
reference's src/with_bundle_adjustment.cpp:196-208, :615-628 and :683-718), the inputs of
tests/test_window_poses_ref.py, and the gate scenes of tests/test_window_poses.py.

Nothing here shares code with the library: the chain multiplies by numpy.linalg.inv of T = [R | s t], the blocks come
from numpy.linalg.inv of the pose and a log map through arctan2(|v|, tr R - 1) with the axis from the antisymmetric
part (from the symmetric part near pi) -- the library goes through closed-form inverses and the unit quaternion.
Every function takes a dtype, so that the tolerance can be measured: the same restatement in numpy.longdouble (there
with a Gauss-Jordan inverse written out below, numpy.linalg has none for it)."""
import math

import numpy as np

import landmarks_ref as LR

OK, NONFINITE = range(2)
CONVERGENCE, NO_CONVERGENCE, FAILURE, SKIPPED = range(4)
MAX_ROT_DIFF, MAX_TRANS_DIFF = 0.5, 50.0

# 16 x the largest absolute difference between this restatement in float64 and in longdouble over cases() and
# gate_cases_plain(), as tests/test_window_poses_ref.py measures it (it asserts that what it measures is not above
# this value).  The margin: two correctly rounded chains of up to 7 products may differ by more than one run shows.
# Measured: the largest difference is 3.93e-14 (poses of magnitude up to a few tens), 16 x = 6.29e-13.
TOLERANCE = 16 * 3.94e-14


def inverse(M, dtype):
    """numpy.linalg.inv in float64; Gauss-Jordan with partial pivoting in any other dtype."""
    M = np.array(M, dtype)
    if dtype == np.float64:
        return np.linalg.inv(M)
    n = len(M)
    A = np.concatenate([M, np.eye(n, dtype=dtype)], axis=1)
    for c in range(n):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        A[[c, p]] = A[[p, c]]
        A[c] = A[c] / A[c, c]
        for r in range(n):
            if r != c:
                A[r] = A[r] - A[r, c] * A[c]
    return A[:, n:]


def log_map(R, dtype):
    """Rotation vector of R, angle in [0, pi]."""
    R = np.array(R, dtype)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], dtype)
    nv = np.sqrt(np.sum(v * v))
    angle = np.arctan2(nv, np.trace(R) - dtype(1))
    if angle < dtype(1e-4):  # sin(angle) / angle = 1 - angle^2 / 6 + ...
        return v / (dtype(2) * (dtype(1) - angle * angle / dtype(6)))
    if angle < dtype(math.pi - 1e-3):
        return v / nv * angle
    S = (R + R.T) / dtype(2)  # cos I + (1 - cos) a a^T
    c = np.cos(angle)
    i = int(np.argmax(np.diag(S)))
    a = (S[:, i] - c * np.eye(3, dtype=dtype)[:, i]) / (dtype(1) - c)
    a = a / np.sqrt(np.sum(a * a))
    if np.sum(a * v) < 0:
        a = -a
    return a * angle


def exp_map(w, dtype):
    w = np.array(w, dtype)
    th = np.sqrt(np.sum(w * w))
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype)
    if th < dtype(1e-12):
        return np.eye(3, dtype=dtype) + W
    k = W / th
    return np.eye(3, dtype=dtype) + np.sin(th) * k + (dtype(1) - np.cos(th)) * (k @ k)


def block(C, dtype):
    Ti = inverse(C, dtype)
    return np.concatenate([log_map(Ti[:3, :3], dtype), Ti[:3, 3]])


def chain(T0, R, t, scale, dtype=np.float64):
    """One window.  T0 (4, 4) or None, R (n, 3, 3), t (n, 3), scale (n,) -> poses4x4 (n + 1, 4, 4), poses6 (n + 1, 6),
    status."""
    C = np.eye(4, dtype=dtype) if T0 is None else np.array(T0, dtype)
    p4, p6 = [C], [block(C, dtype)]
    for k in range(len(R)):
        T = np.eye(4, dtype=dtype)
        T[:3, :3] = np.array(R[k], dtype)
        T[:3, 3] = dtype(scale[k]) * np.array(t[k], dtype)
        C = C @ inverse(T, dtype)
        p4.append(C), p6.append(block(C, dtype))
    p4, p6 = np.array(p4), np.array(p6)
    fin = bool(np.isfinite(p4.astype(np.float64)).all() and np.isfinite(p6.astype(np.float64)).all())
    return p4, p6, OK if fin else NONFINITE


def gate(solved, built, termination, max_rot=MAX_ROT_DIFF, max_trans=MAX_TRANS_DIFF, dtype=np.float64):
    """One window.  solved / built (L, 6) -> poses4x4 (L, 4, 4), updated (L,), angle (L,), dist (L,)."""
    out, upd, ang, dist = [], [], [], []
    for new, old in zip(np.array(solved, dtype), np.array(built, dtype)):
        Rn, Ro = exp_map(new[:3], dtype), exp_map(old[:3], dtype)
        w = log_map(Rn @ Ro.T, dtype)
        a, d = np.sqrt(np.sum(w * w)), np.sqrt(np.sum((new[3:] - old[3:]) ** 2))
        u = termination == CONVERGENCE and a < max_rot and d < max_trans
        T = np.eye(4, dtype=dtype)
        T[:3, :3], T[:3, 3] = (Rn, new[3:]) if u else (Ro, old[3:])
        out.append(inverse(T, dtype)), upd.append(u), ang.append(a), dist.append(d)
    return np.array(out), np.array(upd, np.uint8), np.array(ang), np.array(dist)


# ---- the inputs of the CPU tests ---------------------------------------------------------------------------------

def rot(axis, angle):
    axis = np.asarray(axis, float)
    return LR.rodrigues(axis / np.linalg.norm(axis) * angle)


def rigid(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def first_poses():
    """identity, a rotation of exactly pi about a tilted axis (the quaternion branch: 1 + tr R = 0), and one of
    1e-9 rad"""
    a = np.array([1.0, 2.0, -2.0]) / 3.0  # a unit vector of rationals: 2 a a^T - I is a rotation of pi
    return {"identity": None, "pi": rigid(2.0 * np.outer(a, a) - np.eye(3), [0.5, -1.0, 2.0]),
            "tiny": rigid(rot([0.3, -1.0, 0.2], 1e-9), [-3.0, 0.25, 1.0])}


def cases():
    """(name, T0, R, t, scale): every first pose with windows of 2, 5 and 8 frames, a scale0 of 0.1 and one of 5,
    and a degenerate pair (R = I, t = 0) in the windows of 5 and 8"""
    out = []
    for name, T0 in first_poses().items():
        for L in (2, 5, 8):
            for s0 in (0.1, 5.0):
                rng = np.random.default_rng(1000 * L + int(10 * s0))
                n = L - 1
                R = np.stack([rot(rng.normal(size=3), math.radians(rng.uniform(0.1, 4.0))) for _ in range(n)])
                t = rng.normal(size=(n, 3))
                t /= np.linalg.norm(t, axis=1)[:, None]
                scale = np.r_[s0, rng.uniform(0.5, 1.5, n - 1)]
                if n >= 3:
                    R[2], t[2] = np.eye(3), 0.0  # the degenerate pose of a pair without five inliers
                out.append(("%s_L%d_s%g" % (name, L, s0), T0, R, t, scale))
    return out


def gate_cases_plain():
    """(solved, built, termination) of windows of 4 poses without any solve: blocks moved by chosen amounts, so that
    with the standard thresholds poses fall on both sides of each, for every termination"""
    rng = np.random.default_rng(5)
    out = []
    for term in (CONVERGENCE, NO_CONVERGENCE, FAILURE, SKIPPED):
        built = np.c_[rng.normal(size=(4, 3)) * 0.4, rng.normal(size=(4, 3)) * 3.0]
        solved = built.copy()
        for i, (da, dt) in enumerate(((0.0, 0.0), (0.3, 10.0), (0.7, 1.0), (0.1, 60.0))):
            Rn = rot(rng.normal(size=3), da) @ LR.rodrigues(built[i, :3]) if da else LR.rodrigues(built[i, :3])
            solved[i, :3] = LR.rotvec(Rn)
            d = rng.normal(size=3)
            solved[i, 3:] = built[i, 3:] + d / np.linalg.norm(d) * dt
        out.append((solved, built, term))
    return out


# ---- the gate scenes of the GPU test: landmarks blocks built from host poses, perturbed as tests/test_ba.py does ----

GATE_SLOTS, GATE_LEN = 60, 4
GATE_ITERS = (200, 1)  # the solves of the gate test: to convergence, and one iteration (NO_CONVERGENCE)


def gate_scenes():
    """Five windows of 4 poses and 60 slots: poses 2 and 3 start 0.002, 0.05, 0.7 and 0.3 rad (and five times as many
    units) off -- from 0.7 rad the solve has to turn a pose by more than MAX_ROT_DIFF to converge --, and a window
    whose first two cameras coincide (ORBX_LM_BASELINE: skipped)"""
    perts = (0.002, 0.05, 0.7, 0.3, 0.01)
    scenes = [LR.make_scene(40 + i, W=GATE_LEN, slots=GATE_SLOTS, min_seen=GATE_LEN, pose_pert=p)
              for i, p in enumerate(perts)]
    poses, tracks, seen = LR.stack(scenes)
    poses[4, 1] = poses[4, 0]  # no baseline
    return poses, tracks, seen


def mid_thresholds(angle, dist, updated_possible):
    """max_rot / max_trans between two poses' values: the midpoint of the two middle values of the poses that could
    be updated (converged windows, poses 1 ..), so that at least one pose falls on each side of each threshold"""
    a, d = np.sort(angle[updated_possible]), np.sort(dist[updated_possible])
    k = len(a) // 2
    return float((a[k - 1] + a[k]) / 2), float((d[k - 1] + d[k]) / 2)
