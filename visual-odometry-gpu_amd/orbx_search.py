"""ctypes binding of include/orbx_search.h, the ninth public header of liborbx.so: the
landmarks of the current block projected into a predicted view, and two described point sets re-associated inside a
position gate, into the `origin` block that orbx_carry.landmarks_carry reads.  The functions take a Context of `orbx`;
the library is the one orbx.load() returns, and this module's own prototype table is applied to it once
(tests/test_orbx_search_abi.py checks it against the header)."""
import ctypes as C

import numpy as np

from . import orbx
from .orbx import _count, _desc, _device_arg, _dp, _f64, _i32, _ip, _ptr, _stream, _sync_uploads
from .orbx_carry import CARRY_BUILT
from .orbx_reloc import _points_arg, _set_arg

PROJ_NONE, PROJ_BEHIND, PROJ_OUTSIDE, PROJ_OK = range(4)

P, I, Z, D = orbx.P, orbx.I, orbx.Z, orbx.D
PROTOTYPES = {
    "orbx_landmarks_project_device": (I, [P, P, P, Z, I, I, I, I, D, P]),
    "orbx_landmarks_project_results_device": (I, [P, P]),
    "orbx_landmarks_project_fetch": (I, [P, I, I, P, P, P, P]),
    "orbx_project_landmarks": (I, [P, P, P, I, I, P, P, I, I, D, P, P, P, P]),
    "orbx_reassociate_gated_device": (I, [P, P, P, P, Z, Z, I, P, P, P, P, I, I, D, D, I, I, I, P]),
    "orbx_reassociate_gated_results_device": (I, [P, P]),
    "orbx_reassociate_gated_fetch": (I, [P, I, I, P]),
    "orbx_reassociate_gated": (I, [P, P, P, P, I, P, P, P, P, I, D, D, I, I, I, P, P, P, P]),
}
EXPORTS = list(PROTOTYPES)  # every symbol include/orbx_search.h declares


class LandmarksProjectionView(C.Structure):
    _fields_ = [("xy", C.c_void_p), ("depth", C.c_void_p), ("state", C.c_void_p), ("count", C.c_void_p),
                ("slot_capacity", C.c_int32), ("n_windows", C.c_int32)]


class ReassociateGatedView(C.Structure):
    _fields_ = [("candidates", C.c_void_p), ("q_capacity", C.c_int32), ("n_windows", C.c_int32)]


_lib = None


def load():
    """The library of orbx.load() with every prototype of PROTOTYPES declared."""
    global _lib
    if _lib is None:
        lib = orbx.load()
        for name, (restype, argtypes) in PROTOTYPES.items():
            f = getattr(lib, name, None)  # (a symbol the library lacks is tests/test_orbx_search_abi.py's to report)
            if f is not None:
                f.restype = restype
                f.argtypes = argtypes
        _lib = lib
    return _lib


def landmarks_project(ctx, K, poses6, width, height, margin_px=0.0, source=CARRY_BUILT, n_windows=None,
                      pose_stride=6, stream=None):
    """orbx_landmarks_project_device: rules P1-P5 on the current landmarks block under one predicted pose per window.
    poses6: (n_windows, 6) float64 as a contiguous torch device tensor or a numpy array (copied to the device), or a
    raw device address with n_windows and pose_stride (in doubles) -- the carried-PnP view's poses6 + 48 *
    (window_len - 1) with pose_stride = 6 * window_len reads every window's last pose in place.  Asynchronous;
    landmarks_project_fetch delivers the block."""
    keep = []
    addr, t, up = _device_arg(poses6, np.float64, lambda a: a.dim() == 2 and a.shape[1] == 6,
                              "poses6 must be (n_windows, 6) float64, contiguous, on the device", keep)
    if t is None:
        if n_windows is None:
            raise ValueError("a raw poses6 address needs n_windows")
    else:
        if n_windows not in (None, t.shape[0]) or pose_stride != 6:
            raise ValueError("n_windows / pose_stride differ from the poses6 tensor")
        n_windows = t.shape[0]
    _sync_uploads(up)
    ctx._sp_keep = keep  # (the tensor: kept alive until the next projection)
    K = _f64(K, (3, 3))
    ctx._chk(load().orbx_landmarks_project_device(ctx._h, _dp(K), addr, pose_stride, n_windows, source, width, height,
                                                  margin_px, _stream(stream)))


def landmarks_project_view(ctx):
    """The device-side block of the last landmarks_project (orbx_landmarks_project_results_device)."""
    v = LandmarksProjectionView()
    ctx._chk(load().orbx_landmarks_project_results_device(ctx._h, C.byref(v)))
    return v


def landmarks_project_fetch(ctx, first=0, n=None):
    """Windows [first, first + n) of the last landmarks_project: a dict of xy (n, slots, 2), depth (n, slots) float64,
    state (n, slots) and count (n) int32."""
    v = landmarks_project_view(ctx)
    n = _count(n, first, v.n_windows)
    m = max(n, 1)
    xy, depth = np.zeros((m, v.slot_capacity, 2)), np.zeros((m, v.slot_capacity))
    state, count = np.zeros((m, v.slot_capacity), np.int32), np.zeros(m, np.int32)
    ctx._chk(load().orbx_landmarks_project_fetch(ctx._h, first, n, _ptr(xy), _ptr(depth), _ptr(state), _ptr(count)))
    return dict(xy=xy[:n], depth=depth[:n], state=state[:n], count=count[:n])


def project_landmarks_host(ctx, points3, slot_of_point, slot_capacity, K, pose6, width, height, margin_px=0.0):
    """orbx_project_landmarks: one old window on host arrays.  Returns a dict of xy (slots, 2), depth, state (slots)
    and count; it runs as a projection of one window."""
    pts, slot = _f64(points3, (-1, 3)), _i32(slot_of_point)
    if len(pts) != len(slot):
        raise ValueError("points3 and slot_of_point differ in length")
    n_old, m = len(pts), max(int(slot_capacity), 1)
    K, pose6 = _f64(K, (3, 3)), _f64(pose6, (6,))
    xy, depth, state, count = np.zeros((m, 2)), np.zeros(m), np.zeros(m, np.int32), C.c_int32(-1)
    ctx._chk(load().orbx_project_landmarks(ctx._h, _dp(pts) if n_old else None, _ip(slot) if n_old else None, n_old,
                                           slot_capacity, _dp(K), _dp(pose6), width, height, margin_px, _ptr(xy),
                                           _ptr(depth), _ptr(state), C.byref(count)))
    return dict(xy=xy, depth=depth, state=state, count=count.value)


def reassociate_gated(ctx, query_desc, query_state, query_xy, train_desc, train_state, train_xy, train_pstate=None,
                      radius_px=20.0, ratio=0.8, max_distance=256, accept_lone=0, unique=1, n_windows=None,
                      q_capacity=None, t_capacity=None, point_stride=None, xy_frame_stride=None, stream=None):
    """orbx_reassociate_gated_device: rules F, K-N, I, J for n_windows (query, train) pairs of described sets with
    positions.  desc / state as orbx_reloc.reassociate takes them (a PointDescriptorsView brings its state and
    sizes); query_xy as orbx_reloc.describe_points takes its points (an (n_windows, slots, 2) float32 tensor or view,
    a numpy array, or a raw address with both strides); train_xy (n_windows, slots, 2) float64 and train_pstate
    (n_windows, slots) int32 as contiguous torch device tensors, numpy arrays or raw addresses -- a
    LandmarksProjectionView's xy and state.  Asynchronous; orbx_reloc.reassociate_fetch and reassociate_gated_fetch
    deliver the blocks."""
    keep = []
    qd, qs, nq, qcap, up_q = _set_arg(query_desc, query_state, n_windows, q_capacity, "query", keep)
    td, ts, nt, tcap, up_t = _set_arg(train_desc, train_state, nq, t_capacity, "train", keep)
    if nq != nt:
        raise ValueError("query and train differ in n_windows")
    qxy, _, ps, fs, up_p = _points_arg(query_xy, nq, qcap, point_stride, xy_frame_stride, keep)
    txy, _, up_x = _device_arg(train_xy, np.float64, lambda a: a.numel() == nq * tcap * 2,
                               "train_xy must be (n_windows, slots, 2) float64, contiguous, on the device", keep)
    tps, _, up_s = _device_arg(train_pstate, np.int32, lambda a: a.numel() == nq * tcap,
                               "train_pstate must be (n_windows, slots) int32, contiguous, on the device", keep)
    _sync_uploads(up_q, up_t, up_p, up_x, up_s)
    ctx._ra_keep = keep  # (the tensors: kept alive until the next re-association)
    ctx._chk(load().orbx_reassociate_gated_device(ctx._h, qd, qs, qxy, ps, fs, qcap, td, ts, txy, tps, tcap, nq,
                                                  radius_px, ratio, max_distance, int(accept_lone), int(unique),
                                                  _stream(stream)))


def reassociate_gated_view(ctx):
    """The device-side candidates of the last reassociate_gated (orbx_reassociate_gated_results_device)."""
    v = ReassociateGatedView()
    ctx._chk(load().orbx_reassociate_gated_results_device(ctx._h, C.byref(v)))
    return v


def reassociate_gated_fetch(ctx, first=0, n=None):
    """Windows [first, first + n) of the last reassociate_gated: candidates (n, q_capacity) int32."""
    v = reassociate_gated_view(ctx)
    n = _count(n, first, v.n_windows)
    cand = np.zeros((max(n, 1), v.q_capacity), np.int32)
    ctx._chk(load().orbx_reassociate_gated_fetch(ctx._h, first, n, _ptr(cand)))
    return cand[:n]


def reassociate_gated_host(ctx, query_desc, query_state, query_xy, train_desc, train_state, train_xy,
                           train_pstate=None, radius_px=20.0, ratio=0.8, max_distance=256, accept_lone=0, unique=1):
    """orbx_reassociate_gated: one window on host arrays.  Returns a dict of origin, dist, candidates (nq) and
    count."""
    qd, td, qs, ts = _desc(query_desc), _desc(train_desc), _i32(query_state), _i32(train_state)
    qxy = np.ascontiguousarray(np.asarray(query_xy, np.float32).reshape(-1, 2))
    txy = _f64(train_xy, (-1, 2))
    tps = None if train_pstate is None else _i32(train_pstate)
    if not len(qd) == len(qs) == len(qxy) or not len(td) == len(ts) == len(txy) or (tps is not None and
                                                                                   len(tps) != len(td)):
        raise ValueError("a desc, its state and its positions differ in length")
    nq, nt = len(qd), len(td)
    m = max(nq, 1)
    origin, dist, cand, count = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.int32), C.c_int32(-1)
    ctx._chk(load().orbx_reassociate_gated(ctx._h, _ptr(qd) if nq else None, _ip(qs) if nq else None,
                                           _ptr(qxy) if nq else None, nq, _ptr(td) if nt else None,
                                           _ip(ts) if nt else None, _dp(txy) if nt else None,
                                           None if tps is None or not nt else _ip(tps), nt, radius_px, ratio,
                                           max_distance, int(accept_lone), int(unique), _ptr(origin), _ptr(dist),
                                           C.byref(count), _ptr(cand)))
    return dict(origin=origin[:nq], dist=dist[:nq], candidates=cand[:nq], count=count.value)
