"""Independent float64 numpy reference of the P3P minimal solver and the synthetic scenes of
tests/test_pnp_ref.py.

Nothing here shares code or method with csrc/orbx_pnp_math.h.  The header substitutes u = N(v) / D(v) into one conic,
isolates the quartic's positive roots by bisection on the pieces its derivatives cut and builds R from two orthonormal
triads.  Here the quartic is the Sylvester resultant of the two conics in u (numpy.polymul on coefficient arrays), its
roots are the eigenvalues of the companion matrix (numpy.roots), u comes from the quadratic's common root, and (R, t)
from the Kabsch alignment of the two triangles (numpy.linalg.svd)."""
import math

import numpy as np

from landmarks_ref import K_KITTI, rodrigues

NEAR_DOUBLE = 1e-3    # a kept root this close (relative to max(1, |v|)) to another root of the quartic, or a complex
#                       pair this close to the positive real axis: the problem is near-degenerate
NEAR_POLE = 1e-4      # |D(v)| of a kept root below this: u = N / D is ill-conditioned
NEAR_COLLINEAR = 2e-2  # the world triangle's smallest angle (rad) below this


def poly(*c):
    """coefficients, highest power first (numpy.polymul's order)"""
    return np.array(c, float)


def kabsch(A, B):
    """the rigid motion with B_i = R A_i + t, least squares"""
    ca, cb = A.mean(0), B.mean(0)
    U, _, Vt = np.linalg.svd((B - cb).T @ (A - ca))
    S = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ S @ Vt
    return R, cb - R @ ca


def p3p(X, xy):
    """X: (3, 3) world points, xy: (3, 2) normalised image points.  Returns (solutions, near_degenerate): a list of
    (R, t) world -> camera with all three depths > 0, in ascending v, and whether the problem is near-degenerate by the
    three constants above."""
    X, xy = np.asarray(X, float), np.asarray(xy, float)
    j = np.c_[xy, np.ones(3)]
    j /= np.linalg.norm(j, axis=1)[:, None]
    ca, cb, cg = j[1] @ j[2], j[0] @ j[2], j[0] @ j[1]
    a2, b2, c2 = np.sum((X[1] - X[2]) ** 2), np.sum((X[0] - X[2]) ** 2), np.sum((X[0] - X[1]) ** 2)
    e = [X[1] - X[0], X[2] - X[1], X[0] - X[2]]
    angles = [math.acos(np.clip(-(e[i] @ e[(i + 1) % 3]) / (np.linalg.norm(e[i]) * np.linalg.norm(e[(i + 1) % 3])),
                                -1, 1)) for i in range(3)]
    near = min(angles) < NEAR_COLLINEAR
    q = poly(1.0, -2.0 * cb, 1.0)  # 1 - 2 cb v + v^2
    # conic 1: b2 (u^2 + v^2 - 2 u v ca) - a2 q = 0;  conic 2: b2 (1 + u^2 - 2 u cg) - c2 q = 0; as A u^2 + B u + C
    A1, B1, C1 = poly(b2), poly(-2.0 * b2 * ca, 0.0), np.polysub(poly(b2, 0.0, 0.0), a2 * q)
    A2, B2, C2 = poly(b2), poly(-2.0 * b2 * cg), np.polysub(poly(b2), c2 * q)
    m = lambda x, y: np.polymul(x, y)
    AF_CD = np.polysub(m(A1, C2), m(C1, A2))
    res = np.polysub(m(AF_CD, AF_CD), m(np.polysub(m(A1, B2), m(B1, A2)), np.polysub(m(B1, C2), m(C1, B2))))
    roots = np.roots(res)
    sols = []
    for i, r in enumerate(roots):
        others = np.delete(roots, i)
        scale = max(1.0, abs(r))
        if abs(r.imag) > 1e-9 * scale or r.real <= 0:
            if r.real > 0 and 0 < abs(r.imag) < NEAR_DOUBLE * scale:
                near = True
            continue
        v = r.real
        if len(others) and np.min(np.abs(others - r)) < NEAR_DOUBLE * scale:
            near = True
        den = np.polyval(np.polysub(m(B1, A2), m(A1, B2)), v)  # (B1 A2 - A1 B2) u = A1 C2 - C1 A2
        if abs(den) < NEAR_POLE * b2 * b2:
            near = True
        if den == 0:
            continue
        u = np.polyval(AF_CD, v) / den
        qv = np.polyval(q, v)
        if not (qv > 0 and u > 0):
            if abs(u) < 1e-3:
                near = True
            continue
        s0 = math.sqrt(b2 / qv)
        C = np.array([s0 * j[0], u * s0 * j[1], v * s0 * j[2]])
        R, t = kabsch(X, C)
        if np.all(np.isfinite(R)) and np.all(np.isfinite(t)) and np.all((X @ R.T + t)[:, 2] > 0):
            sols.append((v, R, t))
    sols.sort(key=lambda s: s[0])
    return [(R, t) for _, R, t in sols], near


def random_pose(rng, max_angle=0.5):
    a = rng.normal(size=3)
    R = rodrigues(a / np.linalg.norm(a) * rng.uniform(0.0, max_angle))
    return R, rng.uniform(-1.0, 1.0, 3)


def p3p_problem(seed, K=K_KITTI):
    """One minimal problem: three points 2 .. 50 units deep in a KITTI-like image, a rotation of up to 0.5 rad.
    Returns X (3, 3) world, xy (3, 2) normalised, (R, t) the true pose."""
    rng = np.random.default_rng(seed)
    R, t = random_pose(rng)
    pix = np.c_[rng.uniform(0, 1241, 3), rng.uniform(0, 376, 3), np.ones(3)]
    cam = (np.linalg.inv(K) @ pix.T).T * rng.uniform(2.0, 50.0, 3)[:, None]
    X = (cam - t) @ R  # rows: R^T (cam - t)
    return X, cam[:, :2] / cam[:, 2:], (R, t)


def scene(seed, n=100, outliers=0.0, K=K_KITTI):
    """A noise-free PnP scene: n points 2 .. 50 deep, a true pose, pixels in float64; `outliers`: that share of the
    observations displaced by 20 .. 100 px.  Returns points3 (n, 3), pixels (n, 2), (R, t), inlier flags (n)."""
    rng = np.random.default_rng(seed)
    R, t = random_pose(rng)
    pix = np.c_[rng.uniform(0, 1241, n), rng.uniform(0, 376, n), np.ones(n)]
    cam = (np.linalg.inv(K) @ pix.T).T * rng.uniform(2.0, 50.0, n)[:, None]
    X = (cam - t) @ R
    p = X @ R.T + t
    uv = np.c_[K[0, 0] * p[:, 0] / p[:, 2] + K[0, 2], K[1, 1] * p[:, 1] / p[:, 2] + K[1, 2]]
    bad = np.zeros(n, bool)
    bad[rng.permutation(n)[:int(round(outliers * n))]] = True
    ang, r = rng.uniform(0, 2 * math.pi, n), rng.uniform(20.0, 100.0, n)
    uv = uv + bad[:, None] * np.c_[r * np.cos(ang), r * np.sin(ang)]
    return X, uv, (R, t), ~bad


def pose_error(pose6, R, t):
    """(rotation angle between pose6's rotation and R in rad, |t - pose6's t|)"""
    Re = rodrigues(pose6[:3])
    c = (np.trace(Re.T @ R) - 1.0) / 2.0
    s = np.linalg.norm(Re - R) / (2.0 * math.sqrt(2.0))  # |Re - R|_F = 2 sqrt(2) sin(angle / 2)
    return 2.0 * math.asin(min(1.0, s)) if c > 0 else math.acos(np.clip(c, -1, 1)), float(np.linalg.norm(pose6[3:] - t))


def solution_distance(a, b):
    """max(|R_a - R_b|_max, |t_a - t_b|_max / max(1, |t_b|))"""
    return max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max() / max(1.0, np.linalg.norm(b[1])))
