"""ctypes binding of include/orbx_lm.h, the third public header of liborbx.so: the landmarks
block of tracked windows built from every view of a track, with a reprojection gate and per-slot diagnostics.  The
functions take a Context of `orbx`; the library is the one orbx.load() returns, and this module's own prototype table
is applied to it once (tests/test_orbx_lm_abi.py checks it against the header)."""
import ctypes as C

import numpy as np

from . import orbx
from .orbx import BaSummary, _dp, _f64, _host_window, _ptr, _stream, _tracks_args, _count

TRI_FIRST_TWO, TRI_WIDEST, TRI_ALL_VIEWS = range(3)
KEPT, SHORT, DEGENERATE, BEHIND, REPROJECTION, NO_WINDOW = range(6)

P, I, D = orbx.P, orbx.I, orbx.D
PROTOTYPES = {
    "orbx_landmarks_build_views_device": (I, [P, P, P, P, I, I, I, P, I, D, P]),
    "orbx_landmarks_views_results_device": (I, [P, P]),
    "orbx_landmarks_views_fetch": (I, [P, I, I, P, P]),
    "orbx_bundle_adjust_tracks_views": (I, [P, P, P, P, I, I, P, D, I, P, P, P, P, I, P, I, D]),
}
EXPORTS = list(PROTOTYPES)  # every symbol include/orbx_lm.h declares


class LandmarksViewsView(C.Structure):
    _fields_ = [("reason", C.c_void_p), ("reproj_px", C.c_void_p), ("slot_capacity", C.c_int32),
                ("n_windows", C.c_int32)]


_lib = None


def load():
    """The library of orbx.load() with every prototype of PROTOTYPES declared."""
    global _lib
    if _lib is None:
        lib = orbx.load()
        for name, (restype, argtypes) in PROTOTYPES.items():
            f = getattr(lib, name, None)  # (a symbol the library lacks is tests/test_orbx_lm_abi.py's to report)
            if f is not None:
                f.restype = restype
                f.argtypes = argtypes
        _lib = lib
    return _lib


def landmarks_build_views(ctx, K, tracks, seen=None, poses=None, tri_mode=TRI_ALL_VIEWS, max_reproj_px=0.0,
                          n_windows=None, slot_capacity=None, window_len=None, stream=None):
    """orbx_landmarks_build_views_device.  The tracks arguments are those of Context.landmarks_build (an
    LkWindowsView, tensors, arrays or raw addresses); poses: host (n_windows, window_len, 6), or None for the poses of
    the last window_poses.  Asynchronous; Context.landmarks_fetch delivers the block, landmarks_views_fetch the
    diagnostics."""
    tracks, seen, n_windows, slot_capacity, window_len, ctx._lm_keep = _tracks_args(
        tracks, seen, n_windows, slot_capacity, window_len)  # (the tensors: kept alive until the next build)
    K = _f64(K, (3, 3))
    if poses is not None:
        poses = _f64(poses, (-1, 6))
        if len(poses) != max(n_windows, 0) * max(window_len, 0):
            raise ValueError("poses must be (n_windows, window_len, 6)")
    ctx._chk(load().orbx_landmarks_build_views_device(ctx._h, _dp(K), tracks, seen, n_windows, slot_capacity,
                                                      window_len, None if poses is None else _dp(poses), tri_mode,
                                                      max_reproj_px, _stream(stream)))


def landmarks_views_view(ctx):
    """The device-side diagnostics of the last views build (orbx_landmarks_views_results_device)."""
    v = LandmarksViewsView()
    ctx._chk(load().orbx_landmarks_views_results_device(ctx._h, C.byref(v)))
    return v


def landmarks_views_fetch(ctx, first=0, n=None):
    """Windows [first, first + n) of the last views build: (reason (n, slots) uint8, reproj_px (n, slots) float32)."""
    v = landmarks_views_view(ctx)
    n = _count(n, first, v.n_windows)
    m = max(n, 1)
    reason, px = np.zeros((m, v.slot_capacity), np.uint8), np.zeros((m, v.slot_capacity), np.float32)
    ctx._chk(load().orbx_landmarks_views_fetch(ctx._h, first, n, _ptr(reason), _ptr(px)))
    return reason[:n], px[:n]


def bundle_adjust_tracks_views(ctx, K, tracks, seen, poses, tri_mode=TRI_ALL_VIEWS, max_reproj_px=0.0,
                               huber_delta=1.0, max_iters=200):
    """orbx_bundle_adjust_tracks_views: Context.bundle_adjust_tracks with the two options.  Returns (poses, summary
    dict, landmarks status, points (N, 3), slot_of_point (N))."""
    tracks, seen, slots, wl = _host_window(tracks, seen)
    K, poses = _f64(K, (3, 3)), _f64(poses, (-1, 6), copy=True)
    if len(poses) != wl:
        raise ValueError("poses must be (window_len, 6)")
    pts = np.zeros((max(slots, 1), 3))
    sop = np.zeros(max(slots, 1), np.int32)
    st, cnt, out = C.c_int32(-1), C.c_int(0), BaSummary()
    ctx._chk(load().orbx_bundle_adjust_tracks_views(ctx._h, _dp(K), _ptr(tracks), _ptr(seen), slots, wl, _dp(poses),
                                                    huber_delta, max_iters, C.byref(st), C.byref(out), _ptr(pts),
                                                    _ptr(sop), slots, C.byref(cnt), tri_mode, max_reproj_px))
    return poses, out.as_dict(), st.value, pts[:cnt.value].copy(), sop[:cnt.value].copy()
