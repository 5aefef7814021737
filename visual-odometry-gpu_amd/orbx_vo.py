"""ctypes binding of include/orbx_vo.h, the second public header of liborbx.so: the poses of
tracked windows chained on the device, the landmarks build that reads them there, and the write-back gate behind the
solve.  The functions take a Context of `orbx`; the library is the one orbx.load() returns, and this module's own
prototype table is applied to it once (tests/test_orbx_vo_abi.py checks it against the header)."""
import ctypes as C

import numpy as np

from . import orbx
from .orbx import OK, BaSummary, OrbxError, _dp, _f64, _host_window, _ptr, _stream, _tracks_args, _count

WP_OK, WP_NONFINITE = range(2)
MAX_ROT_DIFF, MAX_TRANS_DIFF = 0.5, 50.0  # src/with_bundle_adjustment.cpp:708-709

P, I, D, U64 = orbx.P, orbx.I, orbx.D, orbx.U64
PROTOTYPES = {
    "orbx_window_poses_device": (I, [P, P, P, P]), "orbx_window_poses_results_device": (I, [P, P]),
    "orbx_window_poses_fetch": (I, [P, I, I, P, P, P]), "orbx_chain_window_poses": (I, [P, P, P, P, I, P, P]),
    "orbx_landmarks_build_chained_device": (I, [P, P, P, P, I, I, I, P]),
    "orbx_bundle_adjust_write_back_device": (I, [P, D, D, P]),
    "orbx_bundle_adjust_write_back_results_device": (I, [P, P]),
    "orbx_bundle_adjust_write_back_fetch": (I, [P, I, I, P, P]),
    "orbx_window_odometry_tracks": (I, [P, P, P, P, I, I, P, D, D, D, I, U64, D, I, D, D, P, P, P, P, P]),
}
EXPORTS = list(PROTOTYPES)  # every symbol include/orbx_vo.h declares


class WindowPosesView(C.Structure):
    _fields_ = [("poses6", C.c_void_p), ("poses4x4", C.c_void_p), ("status", C.c_void_p), ("window_len", C.c_int32),
                ("n_windows", C.c_int32)]


class BaWriteBackView(C.Structure):
    _fields_ = [("poses4x4", C.c_void_p), ("updated", C.c_void_p), ("window_len", C.c_int32), ("n_windows", C.c_int32)]


_lib = None


def load():
    """The library of orbx.load() with every prototype of PROTOTYPES declared."""
    global _lib
    if _lib is None:
        lib = orbx.load()
        for name, (restype, argtypes) in PROTOTYPES.items():
            f = getattr(lib, name, None)  # (a symbol the library lacks is tests/test_orbx_vo_abi.py's to report)
            if f is not None:
                f.restype = restype
                f.argtypes = argtypes
        _lib = lib
    return _lib


def window_poses(ctx, T0=None, scale0=None, stream=None):
    """orbx_window_poses_device: chains the last tracks_pose block of `ctx`.  T0: (n_windows, 4, 4) camera -> world
    poses of the first frames, None: identity; scale0: (n_windows,) scales of pair 0, None: 1.  Asynchronous;
    window_poses_fetch delivers the block."""
    T0 = None if T0 is None else _f64(T0, (-1, 4, 4))
    scale0 = None if scale0 is None else _f64(scale0, (-1,))
    if T0 is not None or scale0 is not None:
        n = ctx.tracks_pose_view().n_windows
        if (T0 is not None and len(T0) != n) or (scale0 is not None and len(scale0) != n):
            raise ValueError("T0 must be (n_windows, 4, 4) and scale0 (n_windows,)")
    ctx._chk(load().orbx_window_poses_device(ctx._h, None if T0 is None else _dp(T0),
                                             None if scale0 is None else _dp(scale0), _stream(stream)))


def window_poses_view(ctx):
    """The device-side block of the last window_poses (orbx_window_poses_results_device)."""
    v = WindowPosesView()
    ctx._chk(load().orbx_window_poses_results_device(ctx._h, C.byref(v)))
    return v


def window_poses_fetch(ctx, first=0, n=None):
    """Windows [first, first + n) of the last window_poses: dict of poses6 (n, window_len, 6), poses4x4
    (n, window_len, 4, 4) and status (n,)."""
    v = window_poses_view(ctx)
    n = _count(n, first, v.n_windows)
    m = max(n, 1)
    out = dict(poses6=np.zeros((m, v.window_len, 6)), poses4x4=np.zeros((m, v.window_len, 4, 4)),
               status=np.zeros(m, np.int32))
    ctx._chk(load().orbx_window_poses_fetch(ctx._h, first, n, _ptr(out["poses6"]), _ptr(out["poses4x4"]),
                                            _ptr(out["status"])))
    return {k: a[:n] for k, a in out.items()}


def chain_window_poses(T0, R, t, scale):
    """orbx_chain_window_poses: one window on the host.  T0 (4, 4) or None, R (n, 3, 3), t (n, 3), scale (n,):
    (poses4x4 (n + 1, 4, 4), poses6 (n + 1, 6))."""
    T0 = None if T0 is None else _f64(T0, (4, 4))
    R, t, scale = _f64(R, (-1, 3, 3)), _f64(t, (-1, 3)), _f64(scale, (-1,))
    n = len(R)
    if len(t) != n or len(scale) != n:
        raise ValueError("R, t and scale differ in length")
    p4, p6 = np.zeros((n + 1, 4, 4)), np.zeros((n + 1, 6))
    st = load().orbx_chain_window_poses(None if T0 is None else _dp(T0), _dp(R), _dp(t), _dp(scale), n, _dp(p4),
                                        _dp(p6))
    if st != OK:
        raise OrbxError(st, "orbx_chain_window_poses")
    return p4, p6


def landmarks_build_chained(ctx, K, tracks, seen=None, n_windows=None, slot_capacity=None, window_len=None,
                            stream=None):
    """orbx_landmarks_build_chained_device: Context.landmarks_build with the poses of the last window_poses.  The
    tracks arguments are those of landmarks_build (an LkWindowsView, tensors, arrays or raw addresses)."""
    tracks, seen, n_windows, slot_capacity, window_len, ctx._lm_keep = _tracks_args(
        tracks, seen, n_windows, slot_capacity, window_len)  # (the tensors: kept alive until the next build)
    K = _f64(K, (3, 3))
    ctx._chk(load().orbx_landmarks_build_chained_device(ctx._h, _dp(K), tracks, seen, n_windows, slot_capacity,
                                                        window_len, _stream(stream)))


def bundle_adjust_write_back(ctx, max_rot=MAX_ROT_DIFF, max_trans=MAX_TRANS_DIFF, stream=None):
    """orbx_bundle_adjust_write_back_device: the gate on the last solved landmarks block.  Asynchronous;
    bundle_adjust_write_back_fetch delivers the results."""
    ctx._chk(load().orbx_bundle_adjust_write_back_device(ctx._h, max_rot, max_trans, _stream(stream)))


def bundle_adjust_write_back_view(ctx):
    """The device-side block of the last write-back (orbx_bundle_adjust_write_back_results_device)."""
    v = BaWriteBackView()
    ctx._chk(load().orbx_bundle_adjust_write_back_results_device(ctx._h, C.byref(v)))
    return v


def bundle_adjust_write_back_fetch(ctx, first=0, n=None):
    """Windows [first, first + n) of the last write-back: (poses4x4 (n, window_len, 4, 4), updated (n, window_len)
    uint8)."""
    v = bundle_adjust_write_back_view(ctx)
    n = _count(n, first, v.n_windows)
    m = max(n, 1)
    poses, updated = np.zeros((m, v.window_len, 4, 4)), np.zeros((m, v.window_len), np.uint8)
    ctx._chk(load().orbx_bundle_adjust_write_back_fetch(ctx._h, first, n, _ptr(poses), _ptr(updated)))
    return poses[:n], updated[:n]


def window_odometry_tracks(ctx, K, tracks, seen, T0=None, scale0=1.0, prob=0.999, threshold=1.0, pose_max_iters=1000,
                           seed=0, huber_delta=1.0, ba_max_iters=200, max_rot=MAX_ROT_DIFF, max_trans=MAX_TRANS_DIFF):
    """orbx_window_odometry_tracks: one window of host tracks (slots, window_len, 2) and seen (slots) from tracks
    pose to the gated poses.  Returns a dict of poses4x4 (window_len, 4, 4), updated (window_len,), wp_status,
    lm_status and summary."""
    tracks, seen, slots, wl = _host_window(tracks, seen)
    K = _f64(K, (3, 3))
    T0 = None if T0 is None else _f64(T0, (4, 4))
    poses, updated = np.zeros((max(wl, 1), 4, 4)), np.zeros(max(wl, 1), np.uint8)
    wp, lm, out = C.c_int32(-1), C.c_int32(-1), BaSummary()
    ctx._chk(load().orbx_window_odometry_tracks(
        ctx._h, _dp(K), _ptr(tracks), _ptr(seen), slots, wl, None if T0 is None else _dp(T0), scale0, prob, threshold,
        pose_max_iters, seed, huber_delta, ba_max_iters, max_rot, max_trans, _dp(poses), _ptr(updated), C.byref(wp),
        C.byref(lm), C.byref(out)))
    return dict(poses4x4=poses[:wl], updated=updated[:wl], wp_status=wp.value, lm_status=lm.value,
                summary=out.as_dict())
