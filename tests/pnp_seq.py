"""ctypes view of the sequential restatement tests/cpp/pnp_sequential.cpp, compiled by the fixtures of the PnP tests
(test infrastructure; not part of build())."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = np.dtype([("pose6", np.float64, 6), ("inliers", np.int32), ("iters", np.int32), ("n_corr", np.int32),
                   ("status", np.int32), ("rms_px", np.float64)])
OK, SKIPPED, FEW_POINTS, NO_MODEL = range(4)
DEFAULTS = dict(prob=0.99, threshold_px=2.0, max_iters=1000, seed=0, refine_iters=10, min_inliers=4)


def compile_so(tmp):
    out = tmp / "pnp_sequential.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
                           "-o", str(out), os.path.join(ROOT, "tests", "cpp", "pnp_sequential.cpp")])
    lib = C.CDLL(str(out))
    V, I, D, U = C.c_void_p, C.c_int, C.c_double, C.c_uint64
    lib.seq_pnp_problem.restype = None
    lib.seq_pnp_problem.argtypes = [V, I, V, V, D, D, I, U, I, I, V, V]
    lib.seq_pnp_windows.restype = None
    lib.seq_pnp_windows.argtypes = [V, I, I, I] + [V] * 8 + [D, D, I, U, I, I, V, V, V]
    lib.seq_pnp_p3p.restype = I
    lib.seq_pnp_p3p.argtypes = [V, V, V]
    lib.seq_pnp_sample3.restype = I
    lib.seq_pnp_sample3.argtypes = [U, C.c_uint32, C.c_uint32, V]
    lib.seq_pnp_update_niters.restype = I
    lib.seq_pnp_update_niters.argtypes = [D, D, I]
    lib.seq_pnp_problem_seed.restype = U
    lib.seq_pnp_problem_seed.argtypes = [U, C.c_uint32]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _params(kw):
    p = dict(DEFAULTS, **kw)
    return (p["prob"], p["threshold_px"], p["max_iters"], p["seed"], p["refine_iters"], p["min_inliers"])


def p3p(lib, X, xy):
    """pnp_p3p on three world points (3, 3) and their normalised image points (3, 2): a list of (R, t)."""
    X, xy = np.ascontiguousarray(X, np.float64), np.ascontiguousarray(xy, np.float64)
    models = np.zeros((4, 12))
    n = lib.seq_pnp_p3p(_p(X), _p(xy), _p(models))
    return [(models[i, :9].reshape(3, 3).copy(), models[i, 9:].copy()) for i in range(n)]


def problem(lib, K, points3, pixels_xy, **kw):
    """One problem on arrays: dict of pose6, mask, inliers, iters, n_corr, status, rms_px."""
    K = np.ascontiguousarray(K, np.float64)
    pts = np.ascontiguousarray(points3, np.float64).reshape(-1, 3)
    pix = np.ascontiguousarray(pixels_xy, np.float64).reshape(-1, 2)
    n = len(pts)
    rec, mask = np.zeros(1, RECORD), np.zeros(max(n, 1), np.uint8)
    lib.seq_pnp_problem(_p(K), n, _p(pts), _p(pix), *_params(kw), _p(rec), _p(mask))
    r = rec[0]
    return dict(pose6=r["pose6"].copy(), mask=mask[:n], inliers=int(r["inliers"]), iters=int(r["iters"]),
                n_corr=int(r["n_corr"]), status=int(r["status"]), rms_px=float(r["rms_px"]))


def windows(lib, K, block, built, cap, **kw):
    """A batch on a fetched landmarks block (Context.landmarks_fetch's dict, or landmarks_seq.seq_build's) and the
    poses it was built from (n, L, 6): dict of records (n, L - 2), poses6 (n, L, 6), mask (n, L - 2, cap)."""
    K = np.ascontiguousarray(K, np.float64)
    built = np.ascontiguousarray(built, np.float64)
    n, L = built.shape[:2]
    a = {k: np.ascontiguousarray(block[k], t) for k, t in (("status", np.int32), ("point_offset", np.int32),
                                                           ("obs_offset", np.int32), ("points3", np.float64),
                                                           ("obs_point", np.int32), ("obs_pose", np.int32),
                                                           ("obs_xy", np.float64))}
    assert len(a["status"]) == n
    rec, seeded, mask = np.zeros((n, L - 2), RECORD), np.zeros((n, L, 6)), np.zeros((n, L - 2, cap), np.uint8)
    lib.seq_pnp_windows(_p(K), n, L, cap, _p(a["status"]), _p(a["point_offset"]), _p(a["obs_offset"]),
                        _p(a["points3"]), _p(a["obs_point"]), _p(a["obs_pose"]), _p(a["obs_xy"]), _p(built),
                        *_params(kw), _p(rec), _p(seeded), _p(mask))
    return dict(records=rec, poses6=seeded, mask=mask)
