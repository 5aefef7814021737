"""ctypes view of the sequential restatement tests/cpp/lm_sequential.cpp (and of tests/cpp/ba_sequential.cpp), compiled
by the fixtures of the landmark tests (test infrastructure; not part of build())."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP, IP, FP = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_float)
KEYS = ("status", "point_offset", "obs_offset", "points3", "slot_of_point", "obs_point", "obs_pose", "obs_xy")


def compile_so(tmp, name):
    out = tmp / (name + ".so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC",
                           "-o", str(out), os.path.join(ROOT, "tests", "cpp", name + ".cpp")])
    return C.CDLL(str(out))


def seq_build(lib, K, poses, tracks, seen):
    """A batch through seq_lm_build, in the format of Context.landmarks_fetch.  poses (n, W, 6), tracks
    (n, slots, W, 2) float32, seen (n, slots) int32."""
    K = np.ascontiguousarray(K, np.float64)
    poses = np.ascontiguousarray(poses, np.float64)
    tracks = np.ascontiguousarray(tracks, np.float32)
    seen = np.ascontiguousarray(seen, np.int32)
    n, cap, W = tracks.shape[:3]
    assert poses.shape == (n, W, 6) and seen.shape == (n, cap)
    out = dict(status=np.zeros(n, np.int32), point_offset=np.zeros(n + 1, np.int32),
               obs_offset=np.zeros(n + 1, np.int32), points3=np.zeros((n * cap, 3)),
               slot_of_point=np.zeros(n * cap, np.int32), obs_point=np.zeros(n * cap * W, np.int32),
               obs_pose=np.zeros(n * cap * W, np.int32), obs_xy=np.zeros((n * cap * W, 2)))
    lib.seq_lm_build.restype = None
    lib.seq_lm_build.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 11
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lib.seq_lm_build(p(K), n, cap, W, p(poses), p(tracks), p(seen), *[p(out[k]) for k in KEYS])
    N, M = int(out["point_offset"][n]), int(out["obs_offset"][n])
    for k in ("points3", "slot_of_point"):
        out[k] = out[k][:N].copy()
    for k in ("obs_point", "obs_pose", "obs_xy"):
        out[k] = out[k][:M].copy()
    out["pose_offset"] = (np.arange(n + 1) * W).astype(np.int32)
    return out


def window_of(block, w):
    """(points3, slot_of_point, obs_point, obs_pose, obs_xy) of window w of a fetched block."""
    p0, p1 = block["point_offset"][w], block["point_offset"][w + 1]
    o0, o1 = block["obs_offset"][w], block["obs_offset"][w + 1]
    return (block["points3"][p0:p1], block["slot_of_point"][p0:p1], block["obs_point"][o0:o1],
            block["obs_pose"][o0:o1], block["obs_xy"][o0:o1])


def assert_blocks_equal(got, ref):
    """Bit for bit in status, offsets, points, observations and slot_of_point."""
    for k in KEYS + ("pose_offset",):
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.shape == b.shape, (k, a.shape, b.shape)
        if a.dtype.kind == "f":
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), k
        else:
            assert np.array_equal(a, b), k


class Summary(C.Structure):
    _fields_ = [("termination", C.c_int32), ("iterations", C.c_int32), ("successful_steps", C.c_int32),
                ("reserved", C.c_int32), ("initial_cost", C.c_double), ("final_cost", C.c_double)]


def seq_ba(lib, K, poses, pts, obs_point, obs_pose, obs_xy, delta=1.0, max_iters=200):
    """tests/cpp/ba_sequential.cpp's solve of one window: (poses, points, summary dict)."""
    d = lambda a: np.array(np.asarray(a, np.float64), order="C")
    i = lambda a: np.ascontiguousarray(np.asarray(a, np.int32))
    K, poses, pts, xy, op, oq = d(K), d(poses), d(pts), d(obs_xy), i(obs_point), i(obs_pose)
    s = Summary()
    lib.seq_ba.restype = None
    lib.seq_ba(K.ctypes.data_as(DP), len(poses), poses.ctypes.data_as(DP), len(pts), pts.ctypes.data_as(DP), len(op),
               op.ctypes.data_as(IP), oq.ctypes.data_as(IP), xy.ctypes.data_as(DP), C.c_double(delta), max_iters,
               C.byref(s))
    return poses, pts, {k: getattr(s, k) for k in ("termination", "iterations", "successful_steps", "initial_cost",
                                                   "final_cost")}
