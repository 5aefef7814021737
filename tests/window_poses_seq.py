"""ctypes view of the sequential restatement tests/cpp/wp_sequential.cpp, compiled by the fixtures of the window-pose
tests through landmarks_seq.compile_so (test infrastructure; not part of build())."""
import ctypes as C

import numpy as np

import landmarks_seq as LS


def compile_seq(tmp):
    return LS.compile_so(tmp, "wp_sequential")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def seq_chain(lib, T0, scale0, R, t, scale):
    """A batch through seq_wp_chain.  R (n, L - 1, 3, 3), t (n, L - 1, 3), scale (n, L - 1); T0 (n, 4, 4) or None,
    scale0 (n,) or None -> dict of poses6 (n, L, 6), poses4x4 (n, L, 4, 4), status (n,), as window_poses_fetch."""
    d = lambda a: None if a is None else np.ascontiguousarray(a, np.float64)
    T0, scale0, R, t, scale = d(T0), d(scale0), d(R), d(t), d(scale)
    n, L = R.shape[0], R.shape[1] + 1
    assert R.shape == (n, L - 1, 3, 3) and t.shape == (n, L - 1, 3) and scale.shape == (n, L - 1)
    out = dict(poses6=np.zeros((n, L, 6)), poses4x4=np.zeros((n, L, 4, 4)), status=np.zeros(n, np.int32))
    lib.seq_wp_chain.restype = None
    lib.seq_wp_chain.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 8
    lib.seq_wp_chain(n, L, _p(T0), _p(scale0), _p(R), _p(t), _p(scale), _p(out["poses6"]), _p(out["poses4x4"]),
                     _p(out["status"]))
    return out


def seq_gate(lib, solved, built, termination, max_rot, max_trans):
    """A batch through seq_wp_gate.  solved / built (n, L, 6), termination (n,) -> poses4x4 (n, L, 4, 4), updated
    (n, L) uint8, angle (n, L), dist (n, L)."""
    solved, built = np.ascontiguousarray(solved, np.float64), np.ascontiguousarray(built, np.float64)
    term = np.ascontiguousarray(termination, np.int32)
    n, L = solved.shape[:2]
    assert solved.shape == built.shape == (n, L, 6) and term.shape == (n,)
    p4, upd = np.zeros((n, L, 4, 4)), np.zeros((n, L), np.uint8)
    angle, dist = np.zeros((n, L)), np.zeros((n, L))
    lib.seq_wp_gate.restype = None
    lib.seq_wp_gate.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double] + \
        [C.c_void_p] * 4
    lib.seq_wp_gate(n, L, _p(solved), _p(built), _p(term), max_rot, max_trans, _p(p4), _p(upd), _p(angle), _p(dist))
    return p4, upd, angle, dist


def solve_scenes(lm_lib, ba_lib, K, poses, tracks, seen, iters=(200, 1)):
    """A batch through the sequential build (lm_sequential) and, per window and per max_iters of `iters`, the
    sequential solve (ba_sequential): (built poses (n, L, 6), {max_iters: solved poses}, {max_iters: terminations (n,)},
    landmarks status (n,)).  A window that is not OK is SKIPPED and keeps its poses."""
    blk = LS.seq_build(lm_lib, K, poses, tracks, seen)
    solved, term = {}, {}
    for it in iters:
        solved[it], term[it] = np.array(poses, np.float64), np.full(len(poses), 3, np.int32)
        for w in range(len(poses)):
            if blk["status"][w] != 0:
                continue
            p3, _, op, oq, xy = LS.window_of(blk, w)
            solved[it][w], _, s = LS.seq_ba(ba_lib, K, poses[w], p3, op, oq, xy, 1.0, it)
            term[it][w] = s["termination"]
    return np.array(poses, np.float64), solved, term, blk["status"]


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
