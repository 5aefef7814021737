"""ctypes view of the sequential restatement tests/cpp/st_sequential.cpp, compiled by the fixtures of the stitch tests
through landmarks_seq.compile_so (test infrastructure; not part of build())."""
import ctypes as C

import numpy as np

import landmarks_seq as LS

KEYS = ("trajectory4x4", "owner", "anchors4x4", "lambda", "status")


def compile_seq(tmp):
    return LS.compile_so(tmp, "st_sequential")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def seq_scale0(lib, scale, stride, scale0_first):
    """scale (n, L - 1): the tracks-pose block's scales -> scale0 (n,), what k_st_scale0 writes"""
    scale = np.ascontiguousarray(scale, np.float64)
    n, L = scale.shape[0], scale.shape[1] + 1
    out = np.zeros(n)
    lib.seq_st_scale0.restype = None
    lib.seq_st_scale0.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
    lib.seq_st_scale0(n, L, stride, scale0_first, _p(scale), _p(out))
    return out


def seq_stitch(lib, poses, stride, T_start=None, align_scale=False):
    """poses (n, L, 4, 4) -> the dict of orbx_stream.stitch_fetch"""
    poses = np.ascontiguousarray(poses, np.float64)
    n, L = poses.shape[:2]
    assert poses.shape == (n, L, 4, 4) and 1 <= stride <= L - 1
    T_start = None if T_start is None else np.ascontiguousarray(T_start, np.float64).reshape(4, 4)
    F = (n - 1) * stride + L
    out = {"trajectory4x4": np.zeros((F, 4, 4)), "owner": np.zeros(F, np.int32), "anchors4x4": np.zeros((n, 4, 4)),
           "lambda": np.zeros(n), "status": np.zeros(n, np.int32)}
    lib.seq_st_stitch.restype = None
    lib.seq_st_stitch.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5
    lib.seq_st_stitch(n, L, stride, _p(poses), _p(T_start), int(bool(align_scale)), *[_p(out[k]) for k in KEYS])
    return out


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_stitch_equal(got, ref):
    assert set(got) == set(ref) == set(KEYS)
    for k in KEYS:
        assert bits_equal(got[k], ref[k]), (k, got[k].shape, ref[k].shape)
