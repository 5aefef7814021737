"""Sliding-window bundle adjustment (the reference's src/with_bundle_adjustment.cpp:577-722).

CPU tests pin the sequential restatement (tests/cpp/ba_sequential.cpp, which shares orbx_ba_math.h with the
kernel) against numpy: the restated sin / cos, the analytic Jacobians, noiseless and noisy synthetic windows
against the truth and against an independent dense Levenberg-Marquardt, one Schur step against the full
damped normal equations.  GPU tests pin orbx_bundle_adjust / orbx_bundle_adjust_batch bit for bit against the
restatement.  Measured worst cases are tabulated in DESIGN.md §9 rank 7."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# KITTI sequence 00 camera (tests/test_pose.py: K_KITTI)
K_KITTI = np.array([[718.856, 0.0, 607.1928], [0.0, 718.856, 185.2157], [0.0, 0.0, 1.0]])
IMG_W, IMG_H = 1241, 376
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)
CONVERGENCE, NO_CONVERGENCE, FAILURE = 0, 1, 2


class Summary(C.Structure):
    _fields_ = [("termination", C.c_int32), ("iterations", C.c_int32), ("successful_steps", C.c_int32),
                ("reserved", C.c_int32), ("initial_cost", C.c_double), ("final_cost", C.c_double)]


@pytest.fixture(scope="module")
def seq(tmp_path_factory):
    """The sequential restatement, compiled here (test infrastructure; not part of build())."""
    out = tmp_path_factory.mktemp("ba_seq") / "ba_sequential.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
                           "-o", str(out), os.path.join(ROOT, "tests", "cpp", "ba_sequential.cpp")])
    return C.CDLL(str(out))


def _d(a):
    a = np.array(np.asarray(a, np.float64), order="C")
    return a, a.ctypes.data_as(DP)


def _i(a):
    a = np.ascontiguousarray(np.asarray(a, np.int32))
    return a, a.ctypes.data_as(IP)


def seq_ba(lib, win, delta=1.0, max_iters=200, K=K_KITTI):
    (Kc, kp), (poses, pp), (pts, xp) = _d(K), _d(win["poses0"]), _d(win["pts0"])
    (op, opp), (oq, oqp), (xy, xyp) = _i(win["obs_point"]), _i(win["obs_pose"]), _d(win["obs_xy"])
    s = Summary()
    lib.seq_ba(kp, len(poses), pp, len(pts), xp, len(op), opp, oqp, xyp, C.c_double(delta), max_iters, C.byref(s))
    return poses, pts, {k: getattr(s, k) for k in ("termination", "iterations", "successful_steps", "initial_cost",
                                                   "final_cost")}


def seq_first_step(lib, win, radius, delta=1.0, K=K_KITTI):
    (Kc, kp), (poses, pp), (pts, xp) = _d(K), _d(win["poses0"]), _d(win["pts0"])
    (op, opp), (oq, oqp), (xy, xyp) = _i(win["obs_point"]), _i(win["obs_pose"]), _d(win["obs_xy"])
    dpo, dpt = np.zeros_like(poses), np.zeros_like(pts)
    lib.seq_ba_first_step.restype = C.c_int
    ok = lib.seq_ba_first_step(kp, len(poses), pp, len(pts), xp, len(op), opp, oqp, xyp, C.c_double(delta),
                               C.c_double(radius), dpo.ctypes.data_as(DP), dpt.ctypes.data_as(DP))
    assert ok == 1
    return dpo, dpt


# ---- geometry in numpy (independent of the library) ----------------------------------------------------------
def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def rodrigues(v):
    th = np.linalg.norm(v)
    if th < 1e-12:
        return np.eye(3) + hat(v)
    k = hat(np.asarray(v) / th)
    return np.eye(3) + math.sin(th) * k + (1.0 - math.cos(th)) * (k @ k)


def rotvec(R):
    """Angle-axis of a rotation matrix, angle in [0, pi] (through the unit quaternion: stable near pi)."""
    q = np.array([1.0 + R[0, 0] + R[1, 1] + R[2, 2], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    if q[0] < 1e-3:  # near pi: the largest diagonal entry names the axis
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        q = np.zeros(4)
        q[1 + i] = 1.0 + R[i, i] - R[j, j] - R[k, k]
        q[1 + j] = R[i, j] + R[j, i]
        q[1 + k] = R[i, k] + R[k, i]
        q[0] = R[k, j] - R[j, k]
    q = q / np.linalg.norm(q)
    if q[0] < 0:
        q = -q
    s = np.linalg.norm(q[1:])
    if s < 1e-300:
        return np.zeros(3)
    return q[1:] / s * (2.0 * math.atan2(s, q[0]))


def project(K, poses, pts, op, oq):
    R = np.stack([rodrigues(p[:3]) for p in poses])
    p = np.einsum("mij,mj->mi", R[oq], pts[op]) + poses[oq, 3:]
    return np.c_[K[0, 0] * p[:, 0] / p[:, 2] + K[0, 2], K[1, 1] * p[:, 1] / p[:, 2] + K[1, 2]], p


def make_window(seed, W=5, n=200, sigma=0.0, outliers=0.0, rot_pert=0.003, t_pert=0.02, x_pert=0.1, K=K_KITTI,
                min_track=2, world=None, from_frame0=False):
    """A synthetic window: W camera poses along a gently turning path (steps of 0.5-1.5 units, at most 3 degrees
    per step) seen from a world frame with an ARBITRARY rotation (angle uniform in [0, pi]), n landmarks at
    depth 6-40 each tracked over min_track-5 consecutive frames (tracks end, as LK tracks do).  sigma: pixel noise;
    outliers: share of observations moved by 5-50 px.  The start is the truth with poses 1.. and all points
    perturbed; pose 0 stays (it is constant in the problem).  Observations come in shuffled order.
    world = (R, t): that world frame instead of a random one; from_frame0: every track starts in frame 0."""
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=3)
    Rg = rodrigues(axis / np.linalg.norm(axis) * rng.uniform(0.0, math.pi))
    tg = rng.uniform(-20.0, 20.0, 3)
    if world is not None:
        Rg, tg = np.asarray(world[0], float), np.asarray(world[1], float)
    Rwc, c = [np.eye(3)], [np.zeros(3)]
    for _ in range(W - 1):
        a = np.array([rng.uniform(-0.3, 0.3), 1.0, rng.uniform(-0.3, 0.3)])
        dR = rodrigues(a / np.linalg.norm(a) * math.radians(rng.uniform(-3.0, 3.0)))
        step = np.array([rng.uniform(-0.05, 0.05), rng.uniform(-0.02, 0.02), 1.0])
        c.append(c[-1] + Rwc[-1] @ (step / np.linalg.norm(step) * rng.uniform(0.5, 1.5)))
        Rwc.append(Rwc[-1] @ dR)
    Rwc = [Rg @ R for R in Rwc]
    c = [Rg @ x + tg for x in c]
    poses = np.array([np.r_[rotvec(R.T), -R.T @ x] for R, x in zip(Rwc, c)])
    Kinv = np.linalg.inv(K)
    pts, op, oq, xy = [], [], [], []
    while len(pts) < n:
        a = 0 if from_frame0 else int(rng.integers(0, max(W - min_track + 1, 1)))
        L = int(rng.integers(min_track, 6))
        X = c[a] + Rwc[a] @ (Kinv @ np.array([rng.uniform(0, IMG_W), rng.uniform(0, IMG_H), 1.0]) * rng.uniform(6.0, 40.0))
        seen = []
        for i in range(a, min(a + L, W)):
            p = Rwc[i].T @ (X - c[i])
            if p[2] < 0.5:
                break
            u = K @ (p / p[2])
            if not (0 <= u[0] < IMG_W and 0 <= u[1] < IMG_H):
                break
            seen.append((i, u[:2]))
        if len(seen) < min(min_track, W):
            continue
        for i, u in seen:
            op.append(len(pts)), oq.append(i), xy.append(u)
        pts.append(X)
    pts, op, oq, xy = np.array(pts), np.array(op, np.int32), np.array(oq, np.int32), np.array(xy)
    if sigma > 0:
        xy = xy + rng.normal(0.0, sigma, xy.shape)
    if outliers > 0:
        bad = rng.random(len(xy)) < outliers
        ang = rng.uniform(0, 2 * math.pi, len(xy))
        xy = xy + bad[:, None] * (rng.uniform(5.0, 50.0, len(xy))[:, None] * np.c_[np.cos(ang), np.sin(ang)])
    poses0 = poses.copy()
    for i in range(1, W):
        a = rng.normal(size=3)
        R = rodrigues(a / np.linalg.norm(a) * rot_pert) @ rodrigues(poses[i, :3])
        poses0[i] = np.r_[rotvec(R), poses[i, 3:] + rng.normal(0.0, t_pert, 3)]
    pts0 = pts + rng.normal(0.0, x_pert, pts.shape)
    order = rng.permutation(len(op))
    return dict(poses=poses, pts=pts, poses0=poses0, pts0=pts0, obs_point=op[order], obs_pose=oq[order],
                obs_xy=xy[order])


def errors_up_to_scale(win, poses, pts):
    """(largest rotation error in rad, largest camera-centre error, largest point error), the last two after
    fitting the free scale on |c1 - c0| and in units of the true |c1 - c0|."""
    def centres(P):
        return np.array([-rodrigues(p[:3]).T @ p[3:] for p in P])
    ct, ce = centres(win["poses"]), centres(poses)
    base = np.linalg.norm(ct[1] - ct[0])
    s = base / np.linalg.norm(ce[1] - ce[0])
    rot = max(np.linalg.norm(rotvec(rodrigues(a[:3]) @ rodrigues(b[:3]).T)) for a, b in zip(poses, win["poses"]))
    cen = np.max(np.linalg.norm(ce[0] + s * (ce - ce[0]) - ct, axis=1)) / base
    pt = np.max(np.linalg.norm(ce[0] + s * (pts - ce[0]) - win["pts"], axis=1)) / base
    return rot, cen, pt


# ---- an independent dense Levenberg-Marquardt in numpy: full Jacobian, numpy.linalg.solve, no Schur ---------------
def np_system(K, poses, pts, op, oq, xy, delta=1.0, weighted=True):
    """residuals (2M), dense Jacobian over [poses 1.., points], cost -- Jacobian of R(w) X by the right Jacobian of
    SO(3): d(R X) = -R [X]x Jr(w) dw."""
    W, N, M = len(poses), len(pts), len(op)
    uv, p = project(K, poses, pts, op, oq)
    r = uv - xy
    s = np.sum(r * r, axis=1)
    rho = np.where(s <= delta * delta, s, 2 * delta * np.sqrt(np.maximum(s, 1e-300)) - delta * delta)
    wt = np.where(s <= delta * delta, 1.0, np.sqrt(delta / np.sqrt(np.maximum(s, 1e-300)))) if weighted else np.ones(M)
    J = np.zeros((2 * M, 6 * (W - 1) + 3 * N))
    Rs, Jr = [], []
    for q in poses:
        w = q[:3]
        th = np.linalg.norm(w)
        R = rodrigues(w)
        h = hat(w)
        if th < 1e-7:
            jr = np.eye(3) - 0.5 * h
        else:
            jr = np.eye(3) - (1 - math.cos(th)) / th ** 2 * h + (th - math.sin(th)) / th ** 3 * (h @ h)
        Rs.append(R), Jr.append(jr)
    fx, fy = K[0, 0], K[1, 1]
    for m in range(M):
        i, j = oq[m], op[m]
        dproj = np.array([[fx / p[m, 2], 0.0, -fx * p[m, 0] / p[m, 2] ** 2], [0.0, fy / p[m, 2], -fy * p[m, 1] / p[m, 2] ** 2]])
        if i > 0:
            J[2 * m:2 * m + 2, 6 * (i - 1):6 * (i - 1) + 3] = wt[m] * dproj @ (-Rs[i] @ hat(pts[j]) @ Jr[i])
            J[2 * m:2 * m + 2, 6 * (i - 1) + 3:6 * i] = wt[m] * dproj
        J[2 * m:2 * m + 2, 6 * (W - 1) + 3 * j:6 * (W - 1) + 3 * j + 3] = wt[m] * dproj @ Rs[i]
    return (wt[:, None] * r).ravel(), J, 0.5 * float(np.sum(rho))


def np_lm(K, win, delta=1.0, max_iters=200):
    """Ceres' trust-region loop (DESIGN.md rank 7 rules 5-8) on the dense system."""
    poses, pts = win["poses0"].copy(), win["pts0"].copy()
    op, oq, xy = win["obs_point"], win["obs_pose"], win["obs_xy"]
    W = len(poses)
    r, J, cost = np_system(K, poses, pts, op, oq, xy, delta)
    scale = 1.0 / (1.0 + np.sqrt(np.sum(J * J, axis=0)))
    radius, dec = 1e4, 2.0
    for it in range(1, max_iters + 1):
        Js = J * scale
        g = Js.T @ r
        if np.max(np.abs(J.T @ r)) <= 1e-10:
            return poses, pts, cost, "convergence", it - 1
        H = Js.T @ Js
        D = np.clip(np.diag(H), 1e-6, 1e32) / radius
        step = np.linalg.solve(H + np.diag(D), -g)
        ms = Js @ step
        model = -float(ms @ (r + 0.5 * ms))
        d = scale * step
        if not model > 0:
            radius, dec = radius / dec, dec * 2
            continue
        x = np.r_[poses[1:].ravel(), pts.ravel()]
        if np.linalg.norm(d) <= 1e-8 * (np.linalg.norm(x) + 1e-8):
            return poses, pts, cost, "convergence", it
        cp, cx = poses.copy(), pts.copy()
        cp[1:] += d[:6 * (W - 1)].reshape(-1, 6)
        cx += d[6 * (W - 1):].reshape(-1, 3)
        r2, J2, cost2 = np_system(K, cp, cx, op, oq, xy, delta)
        if abs(cost - cost2) <= 1e-6 * cost:
            return poses, pts, cost, "convergence", it
        rel = (cost - cost2) / model
        if np.isfinite(cost2) and rel > 1e-3:
            poses, pts, r, J, cost = cp, cx, r2, J2, cost2
            radius, dec = min(radius / max(1.0 / 3.0, 1.0 - (2 * rel - 1) ** 3), 1e16), 2.0
        else:
            radius, dec = radius / dec, dec * 2
    return poses, pts, cost, "no_convergence", max_iters


def ulps(got, ref):
    return 0.0 if got == ref else abs(got - ref) / math.ulp(ref)


# the suites (seed, W, landmarks): sizes span the issue's 50 .. 2000
NOISELESS = [(s, 5, n) for s, n in zip(range(100, 110), (50, 80, 120, 200, 300, 450, 700, 1000, 1500, 2000))] + \
            [(110, 2, 150), (111, 8, 400), (112, 3, 60)]
# The dense numpy system has 2 M x (24 + 3 N) entries: these stay below 300 landmarks.  Tracks of the noisy suite
# last 3-5 frames (NOISY_MIN_TRACK): a landmark seen twice, once by an outlier, is fitted exactly by a depth that
# runs to infinity -- the cost has an asymptote and no minimiser there, both solvers stop on the function tolerance
# somewhere along it (restatement and numpy apart by up to 7 % over seeds 200-209 with 2-frame tracks), and comparing
# those stops measures nothing.  The 2-frame tracks with outliers stay in the GPU suite, where the comparison is
# bit for bit.
NOISY = [(s, 5, n) for s, n in zip(range(200, 210), (50, 60, 80, 100, 120, 150, 180, 220, 260, 300))]
NOISY_MIN_TRACK = 3
# dropped from the margin check (at most 1 seed in 10), still run and printed: in seed 203 one 3-frame landmark has
# two outliers and runs to infinity all the same (|X| = 2.8e6 in the restatement, 2.3e6 in numpy when they stop);
# the two costs differ by 1.6e-5 along that asymptote
NOISY_DROPPED = {203}


# ---- CPU ------------------------------------------------------------------------------------------------------
def test_restated_sin_cos_within_2_ulp(seq):
    """ba_sincos against math.sin / math.cos on [0, pi] (bound: 2 ulp, as for pose_log); measured worst case
    in DESIGN.md.  The same bound is checked up to the restatement's limit of 1e5 rad."""
    rng = np.random.default_rng(7)
    near = np.array([k * math.pi / 4 for k in range(5)])
    xs = np.concatenate([rng.uniform(0, math.pi, 200_000), near, np.nextafter(near, 0), np.nextafter(near[:4], 4),
                         2.0 ** -np.arange(0, 1000.0, 7), rng.uniform(0, 1e-3, 5000)])
    xs = xs[(xs >= 0) & (xs <= math.pi)]
    far = np.concatenate([rng.uniform(math.pi, 100.0, 50_000), rng.uniform(100.0, 1e5, 50_000)])
    s, c = C.c_double(0), C.c_double(0)
    worst = {}
    for name, arr in (("[0, pi]", xs), ("(pi, 1e5]", far)):
        ws = wc = 0.0
        for x in arr:
            seq.seq_sincos(C.c_double(x), C.byref(s), C.byref(c))
            ws, wc = max(ws, ulps(s.value, math.sin(x))), max(wc, ulps(c.value, math.cos(x)))
        worst[name] = (ws, wc)
    print("sin / cos worst ulp:", worst)
    for name in worst:
        assert max(worst[name]) <= 2.0, worst


def test_analytic_jacobians_match_central_differences(seq):
    """Both branches of the rotation, weights on and off.  Along a parameter axis p = R(w) X + t moves with first,
    second and third derivatives of norm <= A = max(1, |X|) (X is in the world frame: the rotation's derivatives
    scale with |X|, not with the depth).  With a = A / p2 and q = |p| / p2 the third derivative of u = f p0 / p2 is
    bounded by M3 = f (1 + q) (a + 6 a^2 + 6 a^3): the seven terms of the quotient rule, each bounded.  Central
    differences with step h therefore have a truncation error <= h^2 M3 / 6; their rounding error is delta / h,
    where delta <= 16 eps f (1 + q + a) bounds the rounding of one residual (a few roundings of p, amplified by
    f / p2, and a few of the quotient).  That sum, per case, is the bound: it follows from h = 1e-5 and the case's
    geometry and is not tuned.  With weights on, Ceres' corrector scales residual and Jacobian by sqrt(rho') <= 1:
    the weighted Jacobian is compared with sqrt(rho') times the difference quotient of the plain residual.  For the
    small-angle pose w0 the neighbours lie on the general branch; its derivative at w0 differs from the small-angle
    branch's (exactly e_k x X) by the derivative of the exponential's second-order term w x (w x X) / 2, at most
    |w0| |X| in p and so f (1 + q) a |w0| in u: that term is added for those cases."""
    h = 1e-5
    eps = 2.220446049250313e-16
    rng = np.random.default_rng(3)
    Kc, kp = _d(K_KITTI)

    def ev(pose, X, xy, weighted):
        r, Jc, Jp, rho = np.zeros(2), np.zeros(12), np.zeros(6), C.c_double(0)
        seq.seq_obs_eval(kp, _d(pose)[1], _d(X)[1], _d(xy)[1], C.c_double(1.0), int(weighted),
                         r.ctypes.data_as(DP), Jc.ctypes.data_as(DP), Jp.ctypes.data_as(DP), C.byref(rho))
        return r, Jc.reshape(2, 6), Jp.reshape(2, 3), rho.value
    worst = worst_rel = 0.0
    for case in range(400):
        small = case % 4 == 0
        if small:
            w = rng.uniform(-1, 1, 3) * 5e-9
        else:
            a = rng.normal(size=3)
            w = a / np.linalg.norm(a) * rng.uniform(1e-3, math.pi)
        R = rodrigues(w)
        p = np.linalg.inv(K_KITTI) @ np.array([rng.uniform(0, IMG_W), rng.uniform(0, IMG_H), 1.0]) * rng.uniform(6, 40)
        t = rng.uniform(-20, 20, 3)
        X = R.T @ (p - t)
        uv = (K_KITTI @ (p / p[2]))[:2]
        xy = uv + (rng.normal(0, 0.3, 2) if case % 2 else rng.uniform(5, 50) * np.array([0.6, -0.8]))
        pose = np.r_[w, t]
        a_, q_ = max(1.0, np.linalg.norm(X)) / p[2], np.linalg.norm(p) / p[2]
        tol = h * h / 6 * 718.856 * (1 + q_) * (a_ + 6 * a_ ** 2 + 6 * a_ ** 3) + 16 * eps * 718.856 * (1 + q_ + a_) / h
        if small:
            tol += 718.856 * (1 + q_) * a_ * np.linalg.norm(w)
        r0, _, _, rho = ev(pose, X, xy, False)
        s = float(r0 @ r0)
        assert abs(rho - (s if s <= 1 else 2 * math.sqrt(s) - 1)) <= 1e-12 * max(1.0, s)
        for weighted in (False, True):
            wt = 1.0 if (not weighted or s <= 1.0) else math.sqrt(1.0 / math.sqrt(s))
            r, Jc, Jp, _ = ev(pose, X, xy, weighted)
            assert np.allclose(r, wt * r0, rtol=1e-14, atol=0)
            num = np.zeros((2, 9))
            for k in range(9):
                d = np.zeros(9)
                d[k] = h
                rp = ev(pose + d[:6], X + d[6:], xy, False)[0]
                rm = ev(pose - d[:6], X - d[6:], xy, False)[0]
                num[:, k] = wt * (rp - rm) / (2 * h)
            err = float(np.max(np.abs(np.c_[Jc, Jp] - num)))
            assert err <= tol, (case, weighted, err, tol)
            worst, worst_rel = max(worst, err), max(worst_rel, err / tol)
    print("Jacobian worst |analytic - central difference|: %.3g, worst share of its bound: %.3g" % (worst, worst_rel))


# DESIGN.md §9 rank 7, table "noiseless windows": worst cases measured over NOISELESS, and the bounds from them
NOISELESS_COST_RATIO_WORST = 4.07e-17  # final / initial cost (seed 100); bound 1000 x
NOISELESS_ROT_WORST = 9.06e-10         # rad (seed 100); bound 10 x
NOISELESS_CENTRE_WORST = 1.16e-8       # in units of |c1 - c0| (seed 100); bound 10 x
NOISELESS_POINT_WORST = 7.62e-6        # in units of |c1 - c0| (seed 105: a point at depth 40 seen over a short baseline); bound 10 x


def test_noiseless_windows_converge_to_the_truth(seq):
    """Every seed of the suite must end with `convergence` (a condition on the suite's perturbation sizes).
    Bounds: 1000 x the worst cost ratio, 10 x the worst pose / point errors measured over the suite."""
    worst = np.zeros(4)
    for seed, W, n in NOISELESS:
        win = make_window(seed, W, n)
        poses, pts, s = seq_ba(seq, win)
        assert s["termination"] == CONVERGENCE, (seed, s)
        assert np.array_equal(poses[0], win["poses0"][0])  # pose 0 is constant
        e = errors_up_to_scale(win, poses, pts)
        print("noiseless", seed, W, n, s, "ratio %.3g rot %.3g centre %.3g point %.3g" %
              (s["final_cost"] / s["initial_cost"], *e))
        worst = np.maximum(worst, [s["final_cost"] / s["initial_cost"], *e])
    print("noiseless worst: ratio %.3g rot %.3g centre %.3g point %.3g" % tuple(worst))
    assert worst[0] <= 1000 * NOISELESS_COST_RATIO_WORST
    assert worst[1] <= 10 * NOISELESS_ROT_WORST and worst[2] <= 10 * NOISELESS_CENTRE_WORST
    assert worst[3] <= 10 * NOISELESS_POINT_WORST


# the restatement's final cost over numpy's, minus 1: the margin is the function tolerance both loops stop on; the
# worst case measured over the nine seeds kept is 3.7e-10 (DESIGN.md table "noisy windows")
NOISY_MARGIN = 1e-6


def test_noisy_windows_against_dense_numpy_lm(seq):
    """sigma = 0.3 px, 10 % of the observations moved by 5-50 px (the Huber branch is live), against an independent
    dense LM in numpy from the same start.  Both stop when a step changes the cost by less than 1e-6 of it, so the
    restatement's final cost may exceed numpy's by that relative margin and no more.  The restatement converges on
    every seed; NOISY_DROPPED names the one seed left out of the margin check, and why."""
    worst = -1.0
    for seed, W, n in NOISY:
        win = make_window(seed, W, n, sigma=0.3, outliers=0.1, min_track=NOISY_MIN_TRACK)
        poses, pts, s = seq_ba(seq, win)
        assert s["termination"] == CONVERGENCE, (seed, s)
        _, _, cost_np, term, it = np_lm(K_KITTI, win)
        assert term == "convergence", seed
        # the reported cost is the cost of the returned blocks
        assert abs(np_system(K_KITTI, poses, pts, win["obs_point"], win["obs_pose"], win["obs_xy"])[2] - s["final_cost"]) \
            <= 1e-9 * s["final_cost"]
        rel = s["final_cost"] / cost_np - 1.0
        print("noisy", seed, n, "seq %.9g (%d it) numpy %.9g (%d it) rel %.3g" % (s["final_cost"], s["iterations"],
                                                                                   cost_np, it, rel))
        if seed not in NOISY_DROPPED:
            worst = max(worst, rel)
        assert s["final_cost"] < 0.5 * s["initial_cost"]
    print("noisy worst relative excess: %.3g" % worst)
    assert worst <= NOISY_MARGIN, worst


def degenerate_windows():
    """(name, window, kwargs, expected termination or None)"""
    out = []
    w = make_window(300, 5, 120, sigma=0.3)  # landmarks 0 .. 9 keep one observation only
    keep = np.ones(len(w["obs_point"]), bool)
    for j in range(10):
        idx = np.flatnonzero(w["obs_point"] == j)
        keep[idx[1:]] = False
    out.append(("landmarks seen once", {**w, "obs_point": w["obs_point"][keep], "obs_pose": w["obs_pose"][keep],
                                        "obs_xy": w["obs_xy"][keep]}, {}, CONVERGENCE))
    w = make_window(301, 5, 150, sigma=0.3)  # nothing sees pose 2
    keep = w["obs_pose"] != 2
    cnt = np.bincount(w["obs_point"][keep], minlength=150)
    keep &= cnt[w["obs_point"]] > 0
    alive = np.flatnonzero(cnt > 0)
    remap = -np.ones(150, np.int32)
    remap[alive] = np.arange(len(alive))
    out.append(("a pose seen by nothing", {**w, "pts": w["pts"][alive], "pts0": w["pts0"][alive],
                                           "obs_point": remap[w["obs_point"][keep]], "obs_pose": w["obs_pose"][keep],
                                           "obs_xy": w["obs_xy"][keep]}, {}, CONVERGENCE))
    w = make_window(302, 5, 200, sigma=0.3, outliers=0.1, rot_pert=0.05, t_pert=0.5, x_pert=2.0)
    out.append(("iteration limit", w, dict(max_iters=3), NO_CONVERGENCE))
    w = make_window(303, 5, 100, sigma=0.3)  # one point behind camera 0: Ceres accepts it, so do we
    c0 = -rodrigues(w["poses"][0, :3]).T @ w["poses"][0, 3:]
    pts0 = w["pts0"].copy()
    pts0[5] = c0 - (pts0[5] - c0)
    out.append(("a point behind a camera", {**w, "pts0": pts0}, {}, None))
    w = make_window(304, 5, 60)  # an observation at depth exactly 0 at the start: failure
    poses0 = w["poses0"].copy()
    poses0[0] = 0.0
    pts0 = w["pts0"].copy()
    j = w["obs_point"][np.flatnonzero(w["obs_pose"] == 0)[0]]
    pts0[j] = [1.0, 2.0, 0.0]
    out.append(("depth 0 at the start", {**w, "poses0": poses0, "pts0": pts0}, {}, FAILURE))
    w = make_window(305, 5, 60)  # a rotation angle beyond the restated sin / cos
    poses0 = w["poses0"].copy()
    poses0[3, :3] = poses0[3, :3] / np.linalg.norm(poses0[3, :3]) * 2e5
    out.append(("theta out of range", {**w, "poses0": poses0}, {}, FAILURE))
    return out


def test_degenerate_windows(seq):
    for name, w, kw, want in degenerate_windows():
        poses, pts, s = seq_ba(seq, w, **kw)
        print(name, s)
        if want is not None:
            assert s["termination"] == want, (name, s)
        if s["termination"] != CONVERGENCE:  # outputs = inputs (the reference writes back only on CONVERGENCE)
            assert np.array_equal(poses, w["poses0"]) and np.array_equal(pts, w["pts0"]), name
        else:
            assert s["final_cost"] < s["initial_cost"], name
        if name == "iteration limit":
            assert s["iterations"] == 3


# relative difference between the Schur step and the dense solve of the same damped normal equations, measured
SCHUR_REL_WORST = 1.36e-12


def test_schur_step_equals_the_dense_damped_normal_equations(seq):
    """One window, one iteration, radius 1e4: the restatement's step (Jacobi scaling, clamped damping, Schur
    complement, closed-form 3x3 inverses, Cholesky) against numpy.linalg.solve on the full system.
    Bound: 100 x the measured relative difference."""
    worst = 0.0
    for seed, n in ((400, 150), (401, 300)):
        win = make_window(seed, 5, n, sigma=0.3, outliers=0.1)
        dpo, dpt = seq_first_step(seq, win, 1e4)
        r, J, _ = np_system(K_KITTI, win["poses0"], win["pts0"], win["obs_point"], win["obs_pose"], win["obs_xy"])
        scale = 1.0 / (1.0 + np.sqrt(np.sum(J * J, axis=0)))
        Js = J * scale
        H = Js.T @ Js
        step = scale * np.linalg.solve(H + np.diag(np.clip(np.diag(H), 1e-6, 1e32) / 1e4), -Js.T @ r)
        got = np.r_[dpo[1:].ravel(), dpt.ravel()]
        assert np.all(dpo[0] == 0)
        rel = np.linalg.norm(got - step) / np.linalg.norm(step)
        print("schur vs dense", seed, "rel %.3g" % rel)
        worst = max(worst, rel)
    assert worst <= 100 * SCHUR_REL_WORST, worst


# ---- GPU ------------------------------------------------------------------------------------------------------
def gpu_cases():
    """(name, window, kwargs): W in {2, 5, 8}, 1 .. 4096 landmarks, every noise kind, the degenerate cases."""
    cases = []
    seed = 500
    for W in (2, 5, 8):
        for n, sigma, outl in ((1, 0.0, 0.0), (7, 0.3, 0.0), (63, 0.0, 0.0), (256, 0.3, 0.1), (257, 0.3, 0.0),
                               (600, 0.0, 0.0), (1000, 0.3, 0.1), (2000, 0.3, 0.1)):
            cases.append(("W%d n%d s%g o%g" % (W, n, sigma, outl), make_window(seed, W, n, sigma=sigma, outliers=outl), {}))
            seed += 1
    cases.append(("W5 n4096", make_window(seed, 5, 4096, sigma=0.3, outliers=0.1), {}))
    cases.append(("W8 n4096", make_window(seed + 1, 8, 4096, sigma=0.3, outliers=0.05), {}))
    cases.append(("delta 2.5", make_window(seed + 2, 5, 300, sigma=0.5, outliers=0.1), dict(delta=2.5)))
    cases += [(n, w, kw) for n, w, kw, _ in degenerate_windows()]
    return cases


def same(a, b):
    return np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and \
        np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64)) and \
        all(np.float64(a[2][k]).tobytes() == np.float64(b[2][k]).tobytes() for k in b[2])


@pytest.mark.gpu
def test_gpu_bundle_adjust_equals_the_restatement_bit_for_bit(pkg, seq):
    cases = gpu_cases()
    assert len(cases) >= 30
    terms = set()
    with pkg.Context(pkg.default_params("gpu")) as c:
        for name, w, kw in cases:
            got = c.bundle_adjust(K_KITTI, w["poses0"], w["pts0"], w["obs_point"], w["obs_pose"], w["obs_xy"],
                                  huber_delta=kw.get("delta", 1.0), max_iters=kw.get("max_iters", 200))
            ref = seq_ba(seq, w, **kw)
            terms.add(ref[2]["termination"])
            assert same(got, ref), (name, got[2], ref[2])
    assert terms == {CONVERGENCE, NO_CONVERGENCE, FAILURE}


@pytest.mark.gpu
def test_gpu_batch_equals_single_windows_bit_for_bit(pkg):
    """A mixed batch (sizes differ, some windows fail, some do not converge), in two orders and on a pipelined
    context: every window equals the single-window entry."""
    cases = [(n, w) for n, w, kw in gpu_cases() if not kw]
    cases = cases[::2] + [c for c in cases if c[0] in ("depth 0 at the start", "theta out of range")]
    hard = make_window(302, 5, 200, sigma=0.3, outliers=0.1, rot_pert=0.05, t_pert=0.5, x_pert=2.0)
    cases.append(("hard start", hard))
    tup = lambda w: (w["poses0"], w["pts0"], w["obs_point"], w["obs_pose"], w["obs_xy"])
    with pkg.Context(pkg.default_params("gpu")) as c:
        single = [c.bundle_adjust(K_KITTI, *tup(w), max_iters=12) for _, w in cases]
        terms = {s[2]["termination"] for s in single}
        assert terms == {CONVERGENCE, NO_CONVERGENCE, FAILURE}, terms
        fwd = c.bundle_adjust_batch(K_KITTI, [tup(w) for _, w in cases], max_iters=12)
        rev = c.bundle_adjust_batch(K_KITTI, [tup(w) for _, w in cases[::-1]], max_iters=12)[::-1]
        for (name, _), a, b, r in zip(cases, fwd, rev, single):
            assert same(a, r) and same(b, r), name
        # more windows than workgroups: the batch repeated until windows share a workgroup's workspace
        many = [tup(w) for _, w in cases if len(w["pts0"]) <= 300]
        reps = 520 // len(many) + 1
        big = c.bundle_adjust_batch(K_KITTI, many * reps, max_iters=12)
        for k, got in enumerate(big):
            assert same(got, big[k % len(many)]), k
    p = pkg.default_params("gpu")
    with pkg.Context(p) as c:
        c.set_pipelined_batches(True)
        pip = c.bundle_adjust_batch(K_KITTI, [tup(w) for _, w in cases], max_iters=12)
        for (name, _), a, r in zip(cases, pip, single):
            assert same(a, r), name


def invalid_calls(w):
    """(name, kwargs overriding a valid call): each must be refused with ORBX_ERR_INVALID_ARG"""
    op, oq, xy = w["obs_point"], w["obs_pose"], w["obs_xy"]
    nan_pose, nan_pt, inf_xy = w["poses0"].copy(), w["pts0"].copy(), xy.copy()
    nan_pose[2, 1], nan_pt[3, 0], inf_xy[4, 1] = np.nan, np.nan, np.inf
    bad_op, bad_oq, neg_op = op.copy(), oq.copy(), op.copy()
    bad_op[0], bad_oq[0], neg_op[1] = len(w["pts0"]), 5, -1
    Kn = K_KITTI.copy()
    Kn[0, 0] = np.nan
    return [("point index", dict(obs_point=bad_op)), ("negative point index", dict(obs_point=neg_op)),
            ("pose index", dict(obs_pose=bad_oq)),
            ("duplicate", dict(obs_point=np.r_[op, op[:1]], obs_pose=np.r_[oq, oq[:1]], obs_xy=np.r_[xy, xy[:1]])),
            ("one pose", dict(poses=w["poses0"][:1], obs_pose=np.zeros_like(oq))),
            ("nine poses", dict(poses=np.r_[w["poses0"], w["poses0"][:4]])),
            ("delta 0", dict(huber_delta=0.0)), ("delta < 0", dict(huber_delta=-1.0)),
            ("delta nan", dict(huber_delta=float("nan"))), ("max_iters 0", dict(max_iters=0)),
            ("max_iters 1001", dict(max_iters=1001)), ("nan pose", dict(poses=nan_pose)),
            ("nan point", dict(points=nan_pt)), ("inf observation", dict(obs_xy=inf_xy)), ("nan K", dict(K=Kn)),
            ("landmark without observation", dict(points=np.r_[w["pts0"], w["pts0"][:1]]))]


@pytest.mark.gpu
def test_gpu_refusals(pkg):
    w = make_window(600, 5, 40)
    base = dict(K=K_KITTI, poses=w["poses0"], points=w["pts0"], obs_point=w["obs_point"], obs_pose=w["obs_pose"],
                obs_xy=w["obs_xy"], huber_delta=1.0, max_iters=200)
    with pkg.Context(pkg.default_params("gpu")) as c:
        for name, kw in invalid_calls(w):
            with pytest.raises(pkg.OrbxError) as e:
                c.bundle_adjust(**{**base, **kw})
            assert e.value.status == pkg.orbx.ERR_INVALID_ARG, name
        # beyond the landmark cap: ORBX_ERR_UNSUPPORTED, nothing written (the binding hands the entry copies, so
        # the check goes through ctypes on arrays of our own)
        n = 65537
        poses, pts = np.array(w["poses0"]), np.tile(w["pts0"][:1], (n, 1))
        op, oq, xy = np.arange(n, dtype=np.int32), np.zeros(n, np.int32), np.tile(w["obs_xy"][:1], (n, 1))
        keep_p, keep_x = poses.copy(), pts.copy()
        s = pkg.orbx.BaSummary()
        s.termination = 77
        f = c._lib.orbx_bundle_adjust
        st = f(c._h, _d(K_KITTI)[1], 5, poses.ctypes.data_as(DP), n, pts.ctypes.data_as(DP), n, op.ctypes.data_as(IP),
               oq.ctypes.data_as(IP), xy.ctypes.data_as(DP), 1.0, 200, C.byref(s))
        assert st == pkg.orbx.ERR_UNSUPPORTED
        assert np.array_equal(poses, keep_p) and np.array_equal(pts, keep_x) and s.termination == 77
        # the cap itself is admitted
        got = c.bundle_adjust(K_KITTI, w["poses0"], pts[:65536], op[:65536], oq[:65536], xy[:65536], max_iters=2)
        assert got[2]["termination"] in (CONVERGENCE, NO_CONVERGENCE)


# ---- the C++ mirror (host/orb.hpp) -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ba_mirror") / "ba_mirror.bin"
    pk = os.path.join(ROOT, "visual-odometry-gpu_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(pk, "host"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "ba_mirror.cpp"), "-L" + pk, "-lorbx",
                           "-Wl,-rpath," + pk, "-Wl,-rpath,/opt/rocm/lib"])
    return str(exe)


def cam_to_world(pose6):
    R = rodrigues(pose6[:3])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R.T, -R.T @ pose6[3:]
    return T


def run_mirror_ba(mirror, tmp_path, win, name):
    W = len(win["poses0"])
    blob = K_KITTI.astype(np.float64).tobytes() + np.int32(W).tobytes()
    blob += b"".join(cam_to_world(q).astype(np.float64).tobytes() for q in win["poses0"])
    n = len(win["pts0"])
    blob += np.int32(n).tobytes()
    for j in range(n):
        idx = np.flatnonzero(win["obs_point"] == j)
        idx = idx[np.argsort(win["obs_pose"][idx])]
        blob += np.int32(len(idx)).tobytes()
        for o in idx:
            blob += np.int32(win["obs_pose"][o]).tobytes() + win["obs_xy"][o].astype(np.float32).tobytes()
    path = tmp_path / (name + ".bin")
    path.write_bytes(blob)
    r = subprocess.run([mirror, "ba", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    head = lines[0].split()
    info = {head[i]: head[i + 1] for i in range(0, len(head), 2)}
    poses = np.array([[float.fromhex(v) for v in ln.split()[4:]] for ln in lines[1:]]).reshape(W, 4, 4)
    updated = np.array([int(ln.split()[3]) for ln in lines[1:]])
    return info, poses, updated


def py_mirror_ba(ctx, win):
    """build_landmarks + run_bundle_adjustment restated with the Python binding: (expected flags, expected poses)."""
    P0 = win["poses0"]
    R = [rodrigues(q[:3]) for q in P0]
    Rr = R[1] @ R[0].T
    tr = P0[1, 3:] - Rr @ P0[0, 3:]
    n = len(win["pts0"])
    obs = {(int(j), int(i)): win["obs_xy"][k].astype(np.float32) for k, (j, i) in enumerate(zip(win["obs_point"], win["obs_pose"]))}
    tri = [j for j in range(n) if (j, 0) in obs and (j, 1) in obs]
    xyz, valid = ctx.triangulate(np.array([obs[j, 0] for j in tri]), np.array([obs[j, 1] for j in tri]), K_KITTI, Rr, tr)
    X = (xyz.astype(np.float64) - P0[0, 3:]) @ R[0]  # R0^T (x - t0)
    keep = [k for k in range(len(tri)) if valid[k] and X[k, 2] > 0]
    op, oq, xy = [], [], []
    for m, k in enumerate(keep):
        for i in range(len(P0)):
            if (tri[k], i) in obs:
                op.append(m), oq.append(i), xy.append(obs[tri[k], i].astype(np.float64))
    poses, _, summ = ctx.bundle_adjust(K_KITTI, P0, X[keep], op, oq, np.array(xy))
    assert summ["termination"] == CONVERGENCE
    flags, out = [], []
    for i in range(len(P0)):
        angle = np.linalg.norm(rotvec(rodrigues(poses[i, :3]) @ R[i].T))
        ok = angle < 0.5 and np.linalg.norm(poses[i, 3:] - P0[i, 3:]) < 50.0
        flags.append(int(ok))
        out.append(cam_to_world(poses[i] if ok else P0[i]))
    return np.array(flags), np.array(out), summ


@pytest.mark.gpu
def test_gpu_cpp_mirror_build_landmarks_and_run_bundle_adjustment(pkg, mirror, tmp_path):
    """A synthetic window given as tracks from frame 0 (float pixels, as LK returns them).  The expected outcome is
    restated with the Python binding: triangulation of frames 0 / 1, the world-frame depth check, the solve, and
    the reference's gate (angle < 0.5 rad, |dt| < 50) applied in numpy.  `near`: every pose passes the gate and is
    written back, closer to the truth.  `scaled`: the same kind of window in units 60 times as large (steps of
    30-90, inside the reference's baseline gate of 100) whose pose 3 starts 60 units off: the solve moves it back
    by more than 50, so the gate rejects it and it stays bit for bit; the other poses are written back."""
    for name in ("near", "scaled"):
        win = make_window(700, 5, 300, sigma=0.1, world=(np.eye(3), (0.0, 0.0, 0.0)), from_frame0=True)
        if name == "scaled":
            win = {**win, **{k: win[k].copy() for k in ("poses", "poses0", "pts", "pts0")}}
            for k in ("poses", "poses0"):
                win[k][:, 3:] *= 60.0
            win["pts"] *= 60.0
            win["pts0"] *= 60.0
            win["poses0"][3, 3:] += 60.0 * np.array([0.6, 0.0, 0.8])
        start = np.array([cam_to_world(q) for q in win["poses0"]])
        truth = np.array([cam_to_world(q) for q in win["poses"]])
        info, poses, updated = run_mirror_ba(mirror, tmp_path, win, name)
        with pkg.Context(pkg.default_params("gpu")) as c:
            flags, want, summ = py_mirror_ba(c, win)
        print(name, info, updated, flags, summ)
        assert info["built"] == "1" and info["ran"] == "1" and int(info["landmarks"]) > 200
        assert int(info["termination"]) == CONVERGENCE
        assert float.fromhex(info["final"]) < float.fromhex(info["initial"])  # the reprojection cost went down
        assert np.array_equal(updated, flags)
        assert np.allclose(poses, want, rtol=0, atol=1e-6 * max(1.0, np.abs(want).max()))
        if name == "near":
            assert np.all(updated == 1)
            rot = lambda A, B: np.linalg.norm(rotvec(A[:3, :3] @ B[:3, :3].T))
            for i in range(1, 5):
                assert rot(poses[i], truth[i]) < 0.5 * rot(start[i], truth[i]), i
        else:
            assert list(updated) == [1, 1, 1, 0, 1], updated
            assert np.array_equal(poses[3], start[3])


@pytest.mark.gpu
def test_gpu_cpp_mirror_track_points_across_window(pkg, oracle, mirror, tmp_path):
    """The np.roll sequence of tests/test_vo_frontend.py: the content moves by (+3, +1) px per frame.  The tracks
    equal frame-by-frame propagation with Context.lk_track on the live points -- so they end exactly where LK's
    status ends them -- and the surviving ones flow by (3, 1) px per frame."""
    base = oracle.load_kitti(0)
    frames = [np.roll(base, (dy, dx), (0, 1)) for dx, dy in [(0, 0), (3, 1), (6, 2), (9, 3), (12, 4)]]
    h, w = base.shape
    p = pkg.default_params("gpu", nfeatures=600, max_width=w, max_height=h)
    with pkg.Context(p) as c:
        kps = c.detect_and_compute(base)["kps"][:500].astype(np.float32)
    kps = np.r_[kps, np.array([[w - 2.0, h - 2.0], [1.0, 1.0], [w - 1.0, 5.0]], np.float32)]  # corners: soon lost
    path = tmp_path / "lk.bin"
    path.write_bytes(np.array([len(frames), w, h], np.int32).tobytes() + b"".join(f.tobytes() for f in frames) +
                     np.int32(len(kps)).tobytes() + kps.tobytes())
    r = subprocess.run([mirror, "lk", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {}
    for ln in r.stdout.splitlines():
        i, f, x, y = ln.split()
        got.setdefault(int(i), []).append((int(f), float.fromhex(x), float.fromhex(y)))
    want = {i: [(0, float(k[0]), float(k[1]))] for i, k in enumerate(kps)}
    with pkg.Context(pkg.default_params("gpu", nlevels=1, max_width=w, max_height=h)) as c:
        live, pts = np.arange(len(kps)), kps
        for fi in range(1, len(frames)):
            nxt, st, _ = c.lk_track(frames[fi - 1], frames[fi], pts)
            for k, i in enumerate(live):
                if st[k]:
                    want[i].append((fi, float(nxt[k, 0]), float(nxt[k, 1])))
            live, pts = live[st != 0], nxt[st != 0]
    assert got == want
    lengths = np.array([len(t) for t in got.values()])
    assert lengths.min() < len(frames) <= lengths.max() and np.mean(lengths == len(frames)) > 0.8
    for t in got.values():
        if len(t) == len(frames):
            flow = (np.array(t[-1][1:]) - np.array(t[0][1:])) / (len(frames) - 1)
            assert abs(flow[0] - 3) < 0.2 and abs(flow[1] - 1) < 0.2, t
