"""Landmark priors in the window solve, CPU side: the sequential restatement with priors
(tests/cpp/ba_prior_sequential.cpp, which shares only orbx_ba_math.h with the kernel) against

  - the restatement of rank 7 (tests/cpp/ba_sequential.cpp), byte for byte when every weight is 0 or no prior is given;
  - an independent dense Levenberg-Marquardt in numpy with the prior rows in its Jacobian;
  - the truth, with NO scale fit, from a start that is a pure gauge move (the truth scaled by 1.05 about camera 0);
  - the three-line numpy formula of the prior term, bit for bit.

The GPU side is tests/test_prior_gpu.py: the kernel against this restatement bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_ba as B
from test_ba import CONVERGENCE, DP, IP, K_KITTI, Summary, _d, _i, seq  # noqa: F401  (seq: the fixture of rank 7)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
START_GIVEN, START_ANCHOR = 0, 1
CPP = os.path.join(ROOT, "tests", "cpp", "ba_prior_sequential.cpp")
SEQ_FLAGS = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]


@pytest.fixture(scope="module")
def pseq(tmp_path_factory):
    """The restatement with priors, compiled here (test infrastructure; not part of build())."""
    out = tmp_path_factory.mktemp("ba_prior_seq") / "ba_prior_sequential.so"
    subprocess.check_call(SEQ_FLAGS + ["-shared", "-fPIC", "-o", str(out), CPP])
    lib = C.CDLL(str(out))
    lib.seq_prior_cost.restype = C.c_double
    return lib


def seq_ba_prior(lib, win, prior_xyz=None, prior_weight=None, start=START_GIVEN, delta=1.0, max_iters=200, K=K_KITTI):
    """(poses, points, summary dict) of the restatement with priors; prior_xyz / prior_weight None: NULL"""
    (Kc, kp), (poses, pp), (pts, xp) = _d(K), _d(win["poses0"]), _d(win["pts0"])
    (op, opp), (oq, oqp), (xy, xyp) = _i(win["obs_point"]), _i(win["obs_pose"]), _d(win["obs_xy"])
    pa = pw = None
    if prior_xyz is not None:
        (a, pa), (w, pw) = _d(prior_xyz), _d(prior_weight)
        assert a.shape == pts.shape and w.shape == (len(pts),)
    s = Summary()
    lib.seq_ba_prior(kp, len(poses), pp, len(pts), xp, len(op), opp, oqp, xyp, pa, pw, int(start), C.c_double(delta),
                     int(max_iters), C.byref(s))
    return poses, pts, {k: getattr(s, k) for k in ("termination", "iterations", "successful_steps", "initial_cost",
                                                   "final_cost")}


def mixed_priors(win, seed, weights=(0.0, 1e-2, 1.0, 1e6), sigma=0.1):
    """anchors = truth + N(0, sigma), one weight per landmark drawn from `weights`"""
    rng = np.random.default_rng(seed)
    n = len(win["pts"])
    return win["pts"] + rng.normal(0.0, sigma, (n, 3)), rng.choice(np.array(weights, np.float64), n)


# ---- 1. the two restatements tied together -------------------------------------------------------------------------
def test_zero_weights_and_null_priors_equal_the_plain_restatement(seq, pseq):
    """Rule P1: lambda = 0 is no operation, so the restatement with priors -- its own loops, storage and rule 9 --
    returns every byte of tests/cpp/ba_sequential.cpp's: poses, points and summary, on the windows of the GPU suite
    of rank 7 and on the degenerate windows, from both start modes (no positive weight: nothing starts elsewhere)."""
    cases = B.gpu_cases()
    assert len(cases) >= 30
    terms = set()
    for k, (name, w, kw) in enumerate(cases):
        ref = B.seq_ba(seq, w, **kw)
        terms.add(ref[2]["termination"])
        rng = np.random.default_rng(900 + k)
        garbage = rng.normal(0.0, 50.0, w["pts0"].shape)  # anchors under weight 0 are never read into a result
        assert B.same(seq_ba_prior(pseq, w, **kw), ref), name
        assert B.same(seq_ba_prior(pseq, w, garbage, np.zeros(len(garbage)), START_GIVEN, **kw), ref), name
        assert B.same(seq_ba_prior(pseq, w, garbage, np.zeros(len(garbage)), START_ANCHOR, **kw), ref), name
    assert terms == {B.CONVERGENCE, B.NO_CONVERGENCE, B.FAILURE}


# ---- 2. against an independent dense numpy LM ----------------------------------------------------------------------
def np_system_prior(K, poses, pts, op, oq, xy, anchors, weights, delta=1.0):
    """test_ba.np_system with three more rows per anchored landmark: residual sqrt(lambda) (X - A), Jacobian
    sqrt(lambda) I on the landmark's columns, no loss function."""
    r, J, cost = B.np_system(K, poses, pts, op, oq, xy, delta)
    W = len(poses)
    idx = np.flatnonzero(weights > 0)
    rp = np.zeros(3 * len(idx))
    Jp = np.zeros((3 * len(idx), J.shape[1]))
    for m, j in enumerate(idx):
        sq = np.sqrt(weights[j])
        rp[3 * m:3 * m + 3] = sq * (pts[j] - anchors[j])
        Jp[3 * m:3 * m + 3, 6 * (W - 1) + 3 * j:6 * (W - 1) + 3 * j + 3] = sq * np.eye(3)
    return np.r_[r, rp], np.vstack([J, Jp]), cost + 0.5 * float(rp @ rp)


def np_lm_prior(K, win, anchors, weights, delta=1.0, max_iters=200, start=START_GIVEN):
    """test_ba.np_lm's loop (Ceres' trust region, rank 7 rules 5-8) on the system with prior rows."""
    poses, pts = win["poses0"].copy(), win["pts0"].copy()
    if start == START_ANCHOR:
        pts[weights > 0] = anchors[weights > 0]
    op, oq, xy = win["obs_point"], win["obs_pose"], win["obs_xy"]
    W = len(poses)
    r, J, cost = np_system_prior(K, poses, pts, op, oq, xy, anchors, weights, delta)
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
        r2, J2, cost2 = np_system_prior(K, cp, cx, op, oq, xy, anchors, weights, delta)
        if abs(cost - cost2) <= 1e-6 * cost:
            return poses, pts, cost, "convergence", it
        rel = (cost - cost2) / model
        if np.isfinite(cost2) and rel > 1e-3:
            poses, pts, r, J, cost = cp, cx, r2, J2, cost2
            radius, dec = min(radius / max(1.0 / 3.0, 1.0 - (2 * rel - 1) ** 3), 1e16), 2.0
        else:
            radius, dec = radius / dec, dec * 2
    return poses, pts, cost, "no_convergence", max_iters


def test_noisy_windows_with_priors_against_dense_numpy_lm(pseq):
    """The noisy windows of test_ba.NOISY (sigma 0.3 px, 10 % outliers) with anchors = truth + N(0, 0.05) on a random
    half of the landmarks and weights drawn from {0.01, 1, 100}.  The criterion is that of rank 7's test: both loops
    stop when a step changes the cost by less than 1e-6 of it, so the restatement's final cost may exceed numpy's by
    test_ba.NOISY_MARGIN and no more; the termination is `convergence` and the reported cost is the cost of the
    returned blocks, prior included (rule P2).  All ten seeds are in the margin check, the one of
    test_ba.NOISY_DROPPED too (measured worst excess over the ten: 1.3e-14)."""
    worst = -1.0
    for seed, W, n in B.NOISY:
        win = B.make_window(seed, W, n, sigma=0.3, outliers=0.1, min_track=B.NOISY_MIN_TRACK)
        rng = np.random.default_rng(7000 + seed)
        anchors = win["pts"] + rng.normal(0.0, 0.05, win["pts"].shape)
        weights = np.where(rng.random(n) < 0.5, rng.choice([0.01, 1.0, 100.0], n), 0.0)
        assert 0 < np.count_nonzero(weights) < n
        poses, pts, s = seq_ba_prior(pseq, win, anchors, weights)
        assert s["termination"] == CONVERGENCE, (seed, s)
        _, _, cost_np, term, it = np_lm_prior(K_KITTI, win, anchors, weights)
        assert term == "convergence", seed
        back = np_system_prior(K_KITTI, poses, pts, win["obs_point"], win["obs_pose"], win["obs_xy"], anchors, weights)[2]
        assert abs(back - s["final_cost"]) <= 1e-9 * s["final_cost"], seed
        rel = s["final_cost"] / cost_np - 1.0
        print("noisy + prior", seed, n, "seq %.9g (%d it) numpy %.9g (%d it) rel %.3g" %
              (s["final_cost"], s["iterations"], cost_np, it, rel))
        worst = max(worst, rel)
        assert s["final_cost"] < s["initial_cost"]
    print("noisy + prior worst relative excess: %.3g" % worst)
    assert worst <= B.NOISY_MARGIN, worst


# ---- 3. the gauge ----------------------------------------------------------------------------------------------------
GAUGE_WINDOWS = [(100, 5, 40), (101, 3, 60), (102, 8, 80), (103, 2, 50)]  # (seed, W, landmarks), noise-free
GAUGE_SCALE = 1.05


def scaled_start(win, s=GAUGE_SCALE):
    """the truth scaled by s about camera 0: every reprojection stays exact, a pure gauge move"""
    c0 = -B.rodrigues(win["poses"][0, :3]).T @ win["poses"][0, 3:]
    poses0 = win["poses"].copy()
    for i, q in enumerate(win["poses"]):
        R = B.rodrigues(q[:3])
        c = -R.T @ q[3:]
        poses0[i, 3:] = -R @ (c0 + s * (c - c0))
    return {**win, "poses0": poses0, "pts0": c0 + s * (win["pts"] - c0)}


def centres(P):
    return np.array([-B.rodrigues(p[:3]).T @ p[3:] for p in P])


def scale_of(win, poses, pts):
    """the scale of the solution about camera 0 against the truth: the median over landmarks (no fit enters a check)"""
    c0 = centres(win["poses"])[0]
    return float(np.median(np.linalg.norm(pts - c0, axis=1) / np.linalg.norm(win["pts"] - c0, axis=1)))


def direct_errors(win, poses, pts):
    """(largest rotation error in rad, largest camera-centre error, largest point error), compared DIRECTLY: no
    scale is fitted; the last two in units of the true |c1 - c0|."""
    ct, ce = centres(win["poses"]), centres(poses)
    base = np.linalg.norm(ct[1] - ct[0])
    rot = max(np.linalg.norm(B.rotvec(B.rodrigues(a[:3]) @ B.rodrigues(b[:3]).T)) for a, b in zip(poses, win["poses"]))
    return rot, np.max(np.linalg.norm(ce - ct, axis=1)) / base, np.max(np.linalg.norm(pts - win["pts"], axis=1)) / base


def gauge_priors(win, kind):
    n = len(win["pts"])
    w = np.zeros(n)
    if kind == "half":
        w[::2] = 1.0
    elif kind == "tenth":
        w[::10] = 1.0
    else:
        w[:] = 1e6
    return win["pts"].copy(), w


# worst cases measured on the restatement over GAUGE_WINDOWS x the three anchorings x both start modes (the test
# prints every case); the bounds are 10 x these.  DESIGN.md §9 rank 20, table "the gauge"
GAUGE_ROT_WORST = 2.72e-9      # rad
GAUGE_CENTRE_WORST = 1.51e-7   # in units of |c1 - c0|
GAUGE_POINT_WORST = 6.59e-7    # in units of |c1 - c0|
GAUGE_SCALE_WORST = 1.08e-8    # |scale - 1|; whatever is measured, 1e-6 is a condition


def test_priors_fix_the_gauge(seq, pseq):
    """From the truth scaled by 1.05 about camera 0 the plain solve has nothing to do -- the cost is 0 at every scale
    -- and keeps the scale it was given.  With anchors at the truth on half the landmarks (weight 1), on a tenth
    (weight 1) and on all (weight 1e6) the solve ends in `convergence` at scale 1, and poses and points are compared
    with the truth directly, with no scale fit."""
    worst = np.zeros(4)
    for seed, W, n in GAUGE_WINDOWS:
        win = scaled_start(B.make_window(seed, W, n))
        poses, pts, s = B.seq_ba(seq, win)
        assert abs(scale_of(win, poses, pts) - 1.0) > 0.04, (seed, s)
        for kind in ("half", "tenth", "all"):
            anchors, weights = gauge_priors(win, kind)
            for start in (START_GIVEN, START_ANCHOR):
                poses, pts, s = seq_ba_prior(pseq, win, anchors, weights, start)
                assert s["termination"] == CONVERGENCE, (seed, kind, start, s)
                assert np.array_equal(poses[0], win["poses0"][0])  # pose 0 is constant
                e = (*direct_errors(win, poses, pts), abs(scale_of(win, poses, pts) - 1.0))
                print("gauge", seed, W, n, kind, start, s, "rot %.3g centre %.3g point %.3g |scale - 1| %.3g" % e)
                worst = np.maximum(worst, e)
    print("gauge worst: rot %.3g centre %.3g point %.3g |scale - 1| %.3g" % tuple(worst))
    assert worst[3] <= 1e-6
    assert worst[0] <= 10 * GAUGE_ROT_WORST and worst[1] <= 10 * GAUGE_CENTRE_WORST
    assert worst[2] <= 10 * GAUGE_POINT_WORST and worst[3] <= 10 * GAUGE_SCALE_WORST


# ---- 4. the prior functions of orbx_ba_math.h ------------------------------------------------------------------------
def test_prior_functions_are_the_numpy_formula_bit_for_bit(pseq):
    """d = X - A; rho += lambda ((d0 d0 + d1 d1) + d2 d2); V[0], V[3], V[5] += lambda; gp += lambda d -- in numpy
    float64 with the same association, every bit.  lambda = 0 leaves every accumulator's bits, a -0.0 included."""
    rng = np.random.default_rng(11)
    for case in range(2000):
        X, A = rng.normal(0.0, 30.0, 3), rng.normal(0.0, 30.0, 3)
        lam = float(rng.choice([1e-2, 1.0, 100.0, 1e6, rng.uniform(0.0, 10.0) + 1e-300]))
        V0, g0, rho0 = rng.normal(0.0, 1e3, 6), rng.normal(0.0, 1e3, 3), np.array([abs(rng.normal(0.0, 10.0))])
        V, g, rho = V0.copy(), g0.copy(), rho0.copy()
        pseq.seq_prior_accum(_d(X)[1], _d(A)[1], C.c_double(lam), V.ctypes.data_as(DP), g.ctypes.data_as(DP),
                             rho.ctypes.data_as(DP))
        d = X - A
        term = np.float64(lam) * ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        wantV = V0.copy()
        wantV[[0, 3, 5]] = wantV[[0, 3, 5]] + np.float64(lam)
        assert V.tobytes() == wantV.tobytes() and g.tobytes() == (g0 + np.float64(lam) * d).tobytes(), case
        assert rho.tobytes() == (rho0 + term).tobytes(), case
        assert np.float64(pseq.seq_prior_cost(_d(X)[1], _d(A)[1], C.c_double(lam))).tobytes() == term.tobytes(), case
    # lambda = 0: no operation at all, not an addition of zero (-0.0 + 0.0 would be +0.0)
    V0, g0, rho0 = np.array([-0.0, 1.0, -0.0, -0.0, 2.0, -0.0]), np.array([-0.0, -0.0, 3.0]), np.array([-0.0])
    V, g, rho = V0.copy(), g0.copy(), rho0.copy()
    X = np.array([1.0, 2.0, 3.0])
    pseq.seq_prior_accum(_d(X)[1], _d(X)[1], C.c_double(0.0), V.ctypes.data_as(DP), g.ctypes.data_as(DP),
                         rho.ctypes.data_as(DP))
    assert V.tobytes() == V0.tobytes() and g.tobytes() == g0.tobytes() and rho.tobytes() == rho0.tobytes()
    nan_anchor = np.array([np.nan, np.inf, 0.0])  # an anchor under weight 0 is not read into anything
    pseq.seq_prior_accum(_d(X)[1], _d(nan_anchor)[1], C.c_double(0.0), V.ctypes.data_as(DP), g.ctypes.data_as(DP),
                         rho.ctypes.data_as(DP))
    assert V.tobytes() == V0.tobytes() and g.tobytes() == g0.tobytes() and rho.tobytes() == rho0.tobytes()


# ---- 7. the stand-alone driver of the sanitizer run ------------------------------------------------------------------
def write_driver_input(path, wins):
    """windows for tests/cpp/ba_prior_driver.cpp: per window W, N, M (int32), then poses0, pts0, obs_point, obs_pose,
    obs_xy, anchors, weights"""
    blob = np.int32(len(wins)).tobytes() + np.ascontiguousarray(K_KITTI).tobytes()
    for win, anchors, weights in wins:
        blob += np.array([len(win["poses0"]), len(win["pts0"]), len(win["obs_point"])], np.int32).tobytes()
        for a, dt in ((win["poses0"], np.float64), (win["pts0"], np.float64), (win["obs_point"], np.int32),
                      (win["obs_pose"], np.int32), (win["obs_xy"], np.float64), (anchors, np.float64),
                      (weights, np.float64)):
            blob += np.ascontiguousarray(a, dt).tobytes()
    path.write_bytes(blob)


def test_the_stand_alone_driver_equals_the_library(pseq, tmp_path):
    """tests/cpp/ba_prior_driver.cpp is the restatement with a main of its own: the program a host-side sanitizer run
    compiles with -fsanitize=address,undefined.  Here it is built plainly and must print what the shared library
    returns on two windows of the gauge test, every double as a hex float."""
    exe = tmp_path / "ba_prior_driver.bin"
    subprocess.check_call(SEQ_FLAGS + ["-Wall", "-Wextra", "-o", str(exe), CPP,
                                       os.path.join(ROOT, "tests", "cpp", "ba_prior_driver.cpp")])
    wins = []
    for (seed, W, n), kind in zip(GAUGE_WINDOWS[:2], ("half", "all")):
        win = scaled_start(B.make_window(seed, W, n))
        wins.append((win, *gauge_priors(win, kind)))
    write_driver_input(tmp_path / "windows.bin", wins)
    r = subprocess.run([str(exe), str(tmp_path / "windows.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 2 * len(wins)
    for k, (win, anchors, weights) in enumerate(wins):
        poses, pts, s = seq_ba_prior(pseq, win, anchors, weights, START_ANCHOR)
        head = lines[2 * k].split()
        assert [int(v) for v in head[:3]] == [s["termination"], s["iterations"], s["successful_steps"]]
        assert [float.fromhex(v).hex() for v in head[3:]] == [float(s["initial_cost"]).hex(), float(s["final_cost"]).hex()]
        assert [float.fromhex(v).hex() for v in lines[2 * k + 1].split()] == \
            [float(v).hex() for v in np.r_[poses.ravel(), pts.ravel()]]
