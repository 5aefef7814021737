"""ctypes view of the sequential restatement tests/cpp/search_sequential.cpp, compiled by the fixtures of the search
tests (test infrastructure; not part of build()), and the figures tests/test_cpp_search.py measured with it."""
import ctypes as C

import numpy as np

import landmarks_seq as LS

# The largest difference, in pixels and in depth units, between the sequential program and tests/search_ref.py's numpy
# projection on search_ref.projection_scene(), measured on the CPU by tests/test_cpp_search.py; the device is compared
# with numpy at ten times that figure (the margin rank 17 gave its solver).
MEASURED_PX = 1.2e-13  # (1.14e-13: one unit in the last place of a pixel coordinate between 512 and 1024)
TOLERANCE_PX = 10 * MEASURED_PX


def compile_so(tmp):
    return LS.compile_so(tmp, "search_sequential")


def project(lib, block, poses6, K, width, height, margin_px, cap, points=None, pose_stride=6):
    """seq_sp_project on a fetched landmarks block; poses6: a float64 array whose window w starts at w * pose_stride
    doubles.  dict of xy (n, cap, 2), depth (n, cap), state (n, cap) int32, count (n) int32."""
    n = len(block["status"])
    K = np.ascontiguousarray(K, np.float64)
    poses6 = np.ascontiguousarray(poses6, np.float64).reshape(-1)
    assert len(poses6) >= (n - 1) * pose_stride + 6
    src = np.ascontiguousarray(block["points3"] if points is None else points, np.float64).reshape(-1, 3)
    status, pt_off = (np.ascontiguousarray(block[k], np.int32) for k in ("status", "point_offset"))
    slot = np.ascontiguousarray(block["slot_of_point"], np.int32)
    out = dict(xy=np.full((n, cap, 2), -1.0), depth=np.full((n, cap), -1.0), state=np.full((n, cap), -1, np.int32),
               count=np.full(n, -1, np.int32))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lib.seq_sp_project.restype = None
    lib.seq_sp_project.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + \
        [C.c_int, C.c_int, C.c_double] + [C.c_void_p] * 4
    lib.seq_sp_project(p(K), n, cap, p(poses6), pose_stride, p(status), p(pt_off), p(slot), p(src), width, height,
                       float(margin_px), p(out["xy"]), p(out["depth"]), p(out["state"]), p(out["count"]))
    return out


def in_gate(lib, qx, qy, tx, ty, radius_px):
    lib.seq_sp_in_gate.restype = C.c_int
    lib.seq_sp_in_gate.argtypes = [C.c_float, C.c_float, C.c_double, C.c_double, C.c_double]
    return bool(lib.seq_sp_in_gate(float(qx), float(qy), float(tx), float(ty), float(radius_px)))


def hexes(a):
    return [float(v).hex() for v in np.asarray(a, np.float64).ravel()]
