"""Relative pose (rules 1-7) restated in numpy and Python integers.

Written from the rule text and OpenCV's published formulas (five-point.cpp, ptsetreg.cpp); it shares no code with
csrc/orbx_pose_math.h, so a wrong formula there is not wrong here.  Everything is float64 unless a rule says float32,
and every route differs from the header's on purpose: matrix products where the header writes sums, numpy's SVD where
it runs Jacobi, lstsq where it uses normal equations and Cramer's rule, an action matrix and numpy's eigenvalues
where it eliminates to a univariate polynomial and bisects.

Test infrastructure only (tests/test_pose_ref.py)."""
import math

import numpy as np

M64 = (1 << 64) - 1
DBL_MIN = 2.2250738585072014e-308
MAX_DRAWS = 4096
DIST_THRESH = 50.0
SAMPSON_FLAG = 1e-12  # a Sampson error this close (relative) to the float32 rounding boundary at tf is "undecided"
DEPTH_FLAG = 1e-9  # so is a depth this close (relative) to 0 or to DIST_THRESH


# ---- rule 2: samples -----------------------------------------------------------------------------------------------


def mix64(z):
    """splitmix64's output function of z + golden gamma."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, it, d, n):
    h = mix64((seed & M64) ^ mix64(((it << 32) | d) & M64))
    return ((h >> 32) * n) >> 32


def sample(seed, it, n):
    """5 distinct indices in [0, n) of RANSAC iteration `it`: a duplicate takes the next draw; None after 4096 draws."""
    idx = []
    for d in range(MAX_DRAWS):
        v = draw(seed, it, d, n)
        if v not in idx:
            idx.append(v)
            if len(idx) == 5:
                return idx
    return None


# ---- rule 5: RANSACUpdateNumIters ----------------------------------------------------------------------------------


def niters_quotient(p, ep):
    """log(1 - p) / log(1 - (1 - ep)^5) after the clamps, or None where the rule returns before dividing."""
    p = min(max(p, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    denom = 1.0 - (1.0 - ep) ** 5
    if denom < DBL_MIN:
        return None
    return math.log(num), math.log(denom)


def update_niters(p, ep, max_iters):
    q = niters_quotient(p, ep)
    if q is None:
        return 0
    num, denom = q
    if denom >= 0 or -num >= max_iters * (-denom):
        return max_iters
    return int(np.rint(num / denom))


# ---- rule 4: Sampson error -----------------------------------------------------------------------------------------


def homog(x, y):
    x = np.asarray(x, np.float64)
    return np.stack([x, np.asarray(y, np.float64), np.ones_like(x)])


def sampson(E, x1, y1, x2, y2):
    """(x2h^T E x1h)^2 / ((E x1h)_0^2 + (E x1h)_1^2 + (E^T x2h)_0^2 + (E^T x2h)_1^2) per point, in float64, and the same
    cast to float32.  E: (3, 3) or (m, 3, 3); the result is (n,) or (m, n)."""
    E = np.asarray(E, np.float64)
    h1, h2 = homog(x1, y1), homog(x2, y2)
    with np.errstate(all="ignore"):
        Ex1 = E @ h1
        Etx2 = np.swapaxes(E, -1, -2) @ h2
        d = (h2 * Ex1).sum(-2)
        err = d * d / (Ex1[..., 0, :] ** 2 + Ex1[..., 1, :] ** 2 + Etx2[..., 0, :] ** 2 + Etx2[..., 1, :] ** 2)
        return err, err.astype(np.float32)


def sampson_boundary(tf):
    """The float64 value at which float32(err) <= tf changes: half-way from tf to the next float32 above it."""
    tf = np.float32(tf)
    return (float(tf) + float(np.nextafter(tf, np.float32(np.inf)))) / 2.0


def sampson_flagged(err, tf):
    """Pairs whose float64 error lies within SAMPSON_FLAG (relative) of that boundary."""
    b = sampson_boundary(tf)
    with np.errstate(all="ignore"):
        return np.abs(err - b) <= SAMPSON_FLAG * b


# ---- rule 6: decomposeEssentialMat and the cheirality test -----------------------------------------------------------

W_MAT = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


def decompose(E):
    """R1 = U W V^T, R2 = U W^T V^T, t = u3 from numpy's SVD with det U, det V > 0; None for a matrix of rank < 2."""
    E = np.asarray(E, np.float64).reshape(3, 3)
    if not np.isfinite(E).all():
        return None
    U, S, Vt = np.linalg.svd(E)
    if not S[1] > 0:
        return None
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    return U @ W_MAT @ Vt, U @ W_MAT.T @ Vt, U[:, 2].copy()


def depths(R, t, x1, y1, x2, y2):
    """Inhomogeneous linear least squares of each correspondence under P1 = [I | 0], P2 = [R | t], by lstsq on the 4x3
    system; returns the depth in each camera, (n,) and (n,)."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64)
    x1, y1, x2, y2 = (np.atleast_1d(np.asarray(v, np.float64)) for v in (x1, y1, x2, y2))
    z1, z2 = np.full(len(x1), np.nan), np.full(len(x1), np.nan)
    for i in range(len(x1)):
        A = np.array([[1.0, 0.0, -x1[i]], [0.0, 1.0, -y1[i]], R[0] - x2[i] * R[2], R[1] - y2[i] * R[2]])
        b = np.array([0.0, 0.0, x2[i] * t[2] - t[0], y2[i] * t[2] - t[1]])
        if not (np.isfinite(A).all() and np.isfinite(b).all()):
            continue
        X = np.linalg.lstsq(A, b, rcond=None)[0]
        z1[i] = X[2]
        z2[i] = R[2] @ X + t[2]
    return z1, z2


def depth_good(z1, z2):
    with np.errstate(all="ignore"):
        return (z1 > 0) & (z1 < DIST_THRESH) & (z2 > 0) & (z2 < DIST_THRESH)


def depth_flagged(z1, z2):
    with np.errstate(all="ignore"):
        f = np.zeros(len(z1), bool)
        for z in (z1, z2):
            f |= (np.abs(z) <= DEPTH_FLAG) | (np.abs(z - DIST_THRESH) <= DEPTH_FLAG * DIST_THRESH)
        return f


# ---- rule 3: an independent five-point solver (action matrix) ------------------------------------------------------
# Polynomials in (x, y, z) are arrays c[i, j, k], the coefficient of x^i y^j z^k.


def pmul(a, b):
    out = np.zeros(tuple(p + q - 1 for p, q in zip(a.shape, b.shape)))
    for i, j, k in zip(*np.nonzero(a)):
        out[i:i + b.shape[0], j:j + b.shape[1], k:k + b.shape[2]] += a[i, j, k] * b
    return out


def padd(a, b):
    out = np.zeros(tuple(max(p, q) for p, q in zip(a.shape, b.shape)))
    out[:a.shape[0], :a.shape[1], :a.shape[2]] += a
    out[:b.shape[0], :b.shape[1], :b.shape[2]] += b
    return out


# graded order: the ten cubic monomials, then the basis of the quotient ring x2 xy xz y2 yz z2 x y z 1
CUBIC = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3)]
BASIS = [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]


def solve5_ref(x1, y1, x2, y2):
    """Every real essential matrix through five correspondences (x2h^T E x1h = 0), unit Frobenius norm: (m, 3, 3) and
    the condition number of the left 10x10 block (inf with an empty list if the system cannot be solved)."""
    h1, h2 = homog(x1, y1).T, homog(x2, y2).T
    Q = np.einsum("ni,nj->nij", h2, h1).reshape(5, 9)
    if not np.isfinite(Q).all():
        return np.zeros((0, 3, 3)), np.inf
    null = np.linalg.svd(Q)[2][5:].reshape(4, 3, 3)  # E = x X + y Y + z Z + W
    P = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            c = np.zeros((2, 2, 2))
            c[1, 0, 0], c[0, 1, 0], c[0, 0, 1], c[0, 0, 0] = null[:, i, j]
            P[i][j] = c
    neg = lambda a: -a
    det = padd(padd(pmul(P[0][0], padd(pmul(P[1][1], P[2][2]), neg(pmul(P[1][2], P[2][1])))),
                    neg(pmul(P[0][1], padd(pmul(P[1][0], P[2][2]), neg(pmul(P[1][2], P[2][0])))))),
               pmul(P[0][2], padd(pmul(P[1][0], P[2][1]), neg(pmul(P[1][1], P[2][0])))))
    EEt = [[padd(padd(pmul(P[i][0], P[j][0]), pmul(P[i][1], P[j][1])), pmul(P[i][2], P[j][2])) for j in range(3)]
           for i in range(3)]
    tr = padd(padd(EEt[0][0], EEt[1][1]), EEt[2][2])
    cons = [det]
    for i in range(3):
        for j in range(3):
            s = padd(padd(pmul(EEt[i][0], P[0][j]), pmul(EEt[i][1], P[1][j])), pmul(EEt[i][2], P[2][j]))
            cons.append(padd(2.0 * s, neg(pmul(tr, P[i][j]))))
    A = np.array([[c[m] for m in CUBIC + BASIS] for c in cons])
    cond = np.linalg.cond(A[:, :10])
    if not np.isfinite(cond):
        return np.zeros((0, 3, 3)), np.inf
    G = np.linalg.solve(A[:, :10], A[:, 10:])  # cubic monomial k = -G[k] . basis on the solution set
    # multiplication by x on the basis: x * basis[i] = sum_j M[i, j] basis[j]
    M = np.zeros((10, 10))
    for i, (a, b, c) in enumerate(BASIS):
        m = (a + 1, b, c)
        if m in CUBIC:
            M[i] = -G[CUBIC.index(m)]
        else:
            M[i, BASIS.index(m)] = 1.0
    lam, vec = np.linalg.eig(M)
    out = []
    for k in range(10):
        if np.imag(lam[k]) != 0:
            continue
        v = np.real(vec[:, k])
        if v[9] == 0:
            continue
        x, y, z = v[6] / v[9], v[7] / v[9], v[8] / v[9]
        E = x * null[0] + y * null[1] + z * null[2] + null[3]
        nrm = np.linalg.norm(E)
        if np.isfinite(nrm) and nrm > 0:
            out.append(E / nrm)
    return np.array(out).reshape(-1, 3, 3), cond


# ---- rules 1-7: the whole run ----------------------------------------------------------------------------------------


def ref_pose(p1, p2, K, prob, threshold, max_iters, seed, solve5):
    """findEssentialMat(RANSAC) + recoverPose in OpenCV's loop order.  solve5(x1, y1, x2, y2) -> (m, 3, 3) is the
    minimal solver.  Beyond the result it returns `candidates` (the four (R, t, good count, mask)), `cand_good`,
    `flag_sampson` (scored (model, point) pairs within SAMPSON_FLAG of the rounding boundary, the final mask's
    included) and `flag_depth` (triangulated depths within DEPTH_FLAG of 0 or 50)."""
    p1 = np.asarray(p1, np.float32).reshape(-1, 2)
    p2 = np.asarray(p2, np.float32).reshape(-1, 2)
    n = len(p1)
    res = {"E": np.zeros((3, 3)), "R": np.eye(3), "t": np.zeros(3), "mask": np.zeros(n, np.uint8), "inliers": 0,
           "good": 0, "iters": 0, "candidates": [], "cand_good": [0, 0, 0, 0], "flag_sampson": 0, "flag_depth": 0}
    if n < 5:
        return res
    K = np.asarray(K, np.float64).reshape(3, 3)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    with np.errstate(all="ignore"):
        x1 = (p1[:, 0].astype(np.float64) - cx) / fx
        y1 = (p1[:, 1].astype(np.float64) - cy) / fy
        x2 = (p2[:, 0].astype(np.float64) - cx) / fx
        y2 = (p2[:, 1].astype(np.float64) - cy) / fy
    thr = threshold / ((fx + fy) / 2.0)
    tf = np.float32(thr * thr)
    niters, best, bestE = max_iters, 0, None
    i = 0
    while i < niters:
        idx = sample(seed, i, n)
        if idx is not None:
            models = solve5(x1[idx], y1[idx], x2[idx], y2[idx])
            if len(models):
                err, e32 = sampson(models, x1, y1, x2, y2)
                res["flag_sampson"] += int(sampson_flagged(err, tf).sum())
                counts = (e32 <= tf).sum(1)
                for m in range(len(models)):
                    if counts[m] > max(best, 4):
                        best = int(counts[m])
                        bestE = models[m].copy()
                        niters = update_niters(prob, (n - best) / n, niters)
        i += 1
    res["iters"] = i
    if best == 0:
        return res
    err, e32 = sampson(bestE, x1, y1, x2, y2)
    res["flag_sampson"] += int(sampson_flagged(err, tf).sum())
    inl = e32 <= tf
    dec = decompose(bestE)
    if dec is None:
        return res
    R1, R2, t = dec
    for R, tt in ((R1, t), (R2, t), (R1, -t), (R2, -t)):
        good = np.zeros(n, bool)
        z1, z2 = depths(R, tt, x1[inl], y1[inl], x2[inl], y2[inl])
        good[inl] = depth_good(z1, z2)
        res["flag_depth"] += int(depth_flagged(z1, z2).sum())
        res["candidates"].append((R, tt, int(good.sum()), good.astype(np.uint8)))
    res["cand_good"] = [c[2] for c in res["candidates"]]
    ch = int(np.argmax(res["cand_good"]))  # the first candidate with the most good points
    R, tt, g, mask = res["candidates"][ch]
    res.update(E=bestE, R=R, t=tt, mask=mask, inliers=best, good=g)
    return res
