"""ctypes binding of include/orbx_pnp.h, the fifth public header of liborbx.so:
perspective-n-point with RANSAC over the landmarks block of tracked windows, one problem per (window, frame >= 2), the
one problem of host arrays, and the solve seeded with the PnP poses.  The functions take a Context of `orbx`; the
library is the one orbx.load() returns, and this module's own prototype table is applied to it once
(tests/test_orbx_pnp_abi.py checks it against the header)."""
import ctypes as C

import numpy as np

from . import orbx
from .orbx import _count, _dp, _f64, _ptr, _stream

OK, SKIPPED, FEW_POINTS, NO_MODEL = range(4)
MAX_REFINE_ITERS = 20

P, I, D, U64 = orbx.P, orbx.I, orbx.D, orbx.U64
PROTOTYPES = {
    "orbx_pnp_ransac": (I, [P, P, P, I, P, D, D, I, U64, I, I, P, P, P, P, P, P]),
    "orbx_window_poses_pnp_device": (I, [P, D, D, I, U64, I, I, P]),
    "orbx_window_poses_pnp_results_device": (I, [P, P]),
    "orbx_window_poses_pnp_fetch": (I, [P, I, I, P, P]),
    "orbx_window_poses_pnp_mask_fetch": (I, [P, I, I, P, I, P]),
    "orbx_bundle_adjust_landmarks_pnp_device": (I, [P, D, I, P]),
}
EXPORTS = list(PROTOTYPES)  # every symbol include/orbx_pnp.h declares


class PnpRecord(C.Structure):
    _fields_ = [("pose6", C.c_double * 6), ("inliers", C.c_int32), ("iters", C.c_int32), ("n_corr", C.c_int32),
                ("status", C.c_int32), ("rms_px", C.c_double)]


RECORD_DTYPE = np.dtype([("pose6", np.float64, 6), ("inliers", np.int32), ("iters", np.int32), ("n_corr", np.int32),
                         ("status", np.int32), ("rms_px", np.float64)])


class WindowPosesPnpView(C.Structure):
    _fields_ = [("records", C.c_void_p), ("poses6", C.c_void_p), ("mask", C.c_void_p), ("slot_capacity", C.c_int32),
                ("window_len", C.c_int32), ("n_windows", C.c_int32)]


_lib = None
_M64 = (1 << 64) - 1


def load():
    """The library of orbx.load() with every prototype of PROTOTYPES declared."""
    global _lib
    if _lib is None:
        lib = orbx.load()
        for name, (restype, argtypes) in PROTOTYPES.items():
            f = getattr(lib, name, None)  # (a symbol the library lacks is tests/test_orbx_pnp_abi.py's to report)
            if f is not None:
                f.restype = restype
                f.argtypes = argtypes
        _lib = lib
    return _lib


def _mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def problem_seed(seed, k):
    """The seed window_poses_pnp gives the problems of frame k (of every window): what pnp_ransac takes for the same
    problem."""
    return _mix64((seed & _M64) ^ _mix64(k & 0xFFFFFFFF))


def pnp_ransac(ctx, points3, pixels_xy, K, prob=0.99, threshold_px=2.0, max_iters=1000, seed=0, refine_iters=10,
               min_inliers=4):
    """orbx_pnp_ransac: one problem on host arrays.  Returns a dict of pose6 (6), mask (n) uint8, inliers, iters,
    rms_px and status."""
    pts, pix, K = _f64(points3, (-1, 3)), _f64(pixels_xy, (-1, 2)), _f64(K, (3, 3))
    if len(pts) != len(pix):
        raise ValueError("points3 and pixels_xy differ in length")
    n = len(pts)
    pose, mask = np.zeros(6), np.zeros(max(n, 1), np.uint8)
    inl, its, st, rms = C.c_int32(0), C.c_int32(0), C.c_int32(-1), C.c_double(0.0)
    ctx._chk(load().orbx_pnp_ransac(ctx._h, _dp(pts) if n else None, _dp(pix) if n else None, n, _dp(K), prob,
                                    threshold_px, max_iters, seed & _M64, refine_iters, min_inliers, _dp(pose),
                                    _ptr(mask), C.byref(inl), C.byref(its), C.byref(rms), C.byref(st)))
    return dict(pose6=pose, mask=mask[:n], inliers=inl.value, iters=its.value, rms_px=rms.value, status=st.value)


def window_poses_pnp(ctx, prob=0.99, threshold_px=2.0, max_iters=1000, seed=0, refine_iters=10, min_inliers=4,
                     stream=None):
    """orbx_window_poses_pnp_device: every (window, frame >= 2) of the last landmarks block.  Asynchronous;
    window_poses_pnp_fetch delivers the results."""
    ctx._chk(load().orbx_window_poses_pnp_device(ctx._h, prob, threshold_px, max_iters, seed & _M64, refine_iters,
                                                 min_inliers, _stream(stream)))


def window_poses_pnp_view(ctx):
    """The device-side block of the last window_poses_pnp (orbx_window_poses_pnp_results_device)."""
    v = WindowPosesPnpView()
    ctx._chk(load().orbx_window_poses_pnp_results_device(ctx._h, C.byref(v)))
    return v


def window_poses_pnp_fetch(ctx, first=0, n=None, masks=True):
    """Windows [first, first + n) of the last window_poses_pnp: a dict of records (n, window_len - 2) in RECORD_DTYPE,
    poses6 (n, window_len, 6): the seeded poses, and, with masks, masks: a list per window of a list per frame >= 2
    of uint8 arrays, one byte per point of the window."""
    v = window_poses_pnp_view(ctx)
    n = _count(n, first, v.n_windows)
    m, per = max(n, 1), v.window_len - 2
    rec, poses = np.zeros((m, per), RECORD_DTYPE), np.zeros((m, v.window_len, 6))
    ctx._chk(load().orbx_window_poses_pnp_fetch(ctx._h, first, n, _ptr(rec), _ptr(poses)))
    out = dict(records=rec[:n], poses6=poses[:n])
    if masks:
        out["masks"] = [[window_poses_pnp_mask(ctx, first + w, 2 + k, v.slot_capacity) for k in range(per)]
                        for w in range(n)]
    return out


def window_poses_pnp_mask(ctx, window, k, capacity=None):
    """orbx_window_poses_pnp_mask_fetch: the mask of problem (window, k), one byte per point of the window."""
    if capacity is None:
        capacity = window_poses_pnp_view(ctx).slot_capacity
    mask, cnt = np.zeros(max(capacity, 1), np.uint8), C.c_int(0)
    ctx._chk(load().orbx_window_poses_pnp_mask_fetch(ctx._h, window, k, _ptr(mask), capacity, C.byref(cnt)))
    return mask[:cnt.value].copy()


def bundle_adjust_landmarks_pnp(ctx, huber_delta=1.0, max_iters=200, stream=None):
    """orbx_bundle_adjust_landmarks_pnp_device: Context.bundle_adjust_landmarks with the poses copy taken from the
    seeded poses of the last window_poses_pnp.  Asynchronous; Context.bundle_adjust_landmarks_fetch delivers the
    results."""
    ctx._chk(load().orbx_bundle_adjust_landmarks_pnp_device(ctx._h, huber_delta, max_iters, _stream(stream)))
