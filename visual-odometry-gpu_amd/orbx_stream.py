"""ctypes binding of include/orbx_stream.h, the fourth public header of liborbx.so: a stream of
overlapping tracked windows, each chained, solved and gated in a frame of its own, joined into one trajectory on the
device.  The functions take a Context of `orbx`; the library is the one orbx.load() returns, and this module's own
prototype table is applied to it once (tests/test_orbx_stream_abi.py checks it against the header)."""
import ctypes as C

import numpy as np

from . import orbx, orbx_lm, orbx_vo
from .orbx import OK, BaSummary, OrbxError, _count, _device_arg, _dp, _f64, _ptr, _stream, _sync_uploads, _tracks_args

ST_OK, ST_BROKEN, ST_SCALE_UNALIGNED = 0, 1, 2  # bits of status[w]

P, I, D, U64 = orbx.P, orbx.I, orbx.D, orbx.U64
_STREAM_OPTIONS = [P, D, D, D, I, U64, I, D, D, I, D, D, I]  # T_start, scale0_first, prob .. align_scale
PROTOTYPES = {
    "orbx_window_poses_stream_device": (I, [P, I, D, P]),
    "orbx_stitch_windows_device": (I, [P, P, I, I, I, P, I, P]),
    "orbx_stitch_results_device": (I, [P, P]),
    "orbx_stitch_fetch": (I, [P, I, I, P, P, I, I, P, P, P]),
    "orbx_stitch_windows": (I, [P, I, I, I, P, I, P, P, P, P, P]),
    "orbx_stream_odometry_tracks_device": (I, [P, P, P, P, I, I, I, I] + _STREAM_OPTIONS + [P]),
    "orbx_stream_odometry_tracks": (I, [P, P, P, P, I, I, I, I] + _STREAM_OPTIONS + [P, P, P, P, P]),
}
EXPORTS = list(PROTOTYPES)  # every symbol include/orbx_stream.h declares


class StitchView(C.Structure):
    _fields_ = [("trajectory4x4", C.c_void_p), ("owner", C.c_void_p), ("anchors4x4", C.c_void_p),
                ("lambda", C.c_void_p), ("status", C.c_void_p), ("n_frames", C.c_int32), ("n_windows", C.c_int32),
                ("window_len", C.c_int32), ("stride", C.c_int32)]


_lib = None


def load():
    """The library of orbx.load() with every prototype of PROTOTYPES declared."""
    global _lib
    if _lib is None:
        lib = orbx.load()
        for name, (restype, argtypes) in PROTOTYPES.items():
            f = getattr(lib, name, None)  # (a symbol the library lacks is tests/test_orbx_stream_abi.py's to report)
            if f is not None:
                f.restype = restype
                f.argtypes = argtypes
        _lib = lib
    return _lib


def stream_frames(n_windows, window_len, stride):
    """F = (W - 1) * stride + L"""
    return (n_windows - 1) * stride + window_len


def _t_start(T_start):
    return None if T_start is None else _f64(T_start, (4, 4))


def window_poses_stream(ctx, stride, scale0_first=1.0, stream=None):
    """orbx_window_poses_stream_device: orbx_vo.window_poses for a stream -- every window from the identity, pair 0's
    scale of window w >= 1 taken on the device from pair `stride` of window w - 1.  Asynchronous;
    orbx_vo.window_poses_fetch delivers the block."""
    ctx._chk(load().orbx_window_poses_stream_device(ctx._h, stride, scale0_first, _stream(stream)))


def stitch_windows_device(ctx, poses, stride, T_start=None, align_scale=False, n_windows=None, window_len=None,
                          stream=None):
    """orbx_stitch_windows_device.  poses: an orbx_vo.BaWriteBackView or WindowPosesView (the sizes come from it), an
    (n_windows, window_len, 4, 4) float64 torch device tensor or numpy array (copied to the device, and waited for), or
    a raw device address (then with n_windows and window_len).  Asynchronous; stitch_fetch delivers the results."""
    if isinstance(poses, (orbx_vo.BaWriteBackView, orbx_vo.WindowPosesView)):
        poses, n_windows, window_len = poses.poses4x4, poses.n_windows, poses.window_len
    keep = []
    poses, t, uploaded = _device_arg(
        poses, np.float64, lambda t: t.dim() == 4 and tuple(t.shape[2:]) == (4, 4),
        "poses must be (n_windows, window_len, 4, 4) float64, contiguous, on the device", keep)
    if t is None:
        if None in (n_windows, window_len):
            raise ValueError("a raw poses address needs n_windows and window_len")
    elif (n_windows, window_len) not in ((None, None), tuple(t.shape[:2])):
        raise ValueError("n_windows / window_len differ from poses.shape")
    else:
        n_windows, window_len = t.shape[:2]
    _sync_uploads(uploaded)
    ctx._st_keep = keep  # (the tensor: kept alive until the next stitch)
    T_start = _t_start(T_start)
    ctx._chk(load().orbx_stitch_windows_device(ctx._h, poses, n_windows, window_len, stride,
                                               None if T_start is None else _dp(T_start), int(bool(align_scale)),
                                               _stream(stream)))


def stitch_view(ctx):
    """The device-side block of the last stitch (orbx_stitch_results_device)."""
    v = StitchView()
    ctx._chk(load().orbx_stitch_results_device(ctx._h, C.byref(v)))
    return v


def stitch_fetch(ctx, first_frame=0, n_frames=None, first_window=0, n_windows=None):
    """Stream frames [first_frame, first_frame + n_frames) and windows [first_window, first_window + n_windows) of the
    last stitch: dict of trajectory4x4 (n_frames, 4, 4), owner (n_frames,), anchors4x4 (n_windows, 4, 4), lambda
    (n_windows,) and status (n_windows,)."""
    v = stitch_view(ctx)
    nf, nw = _count(n_frames, first_frame, v.n_frames), _count(n_windows, first_window, v.n_windows)
    mf, mw = max(nf, 1), max(nw, 1)
    out = {"trajectory4x4": np.zeros((mf, 4, 4)), "owner": np.zeros(mf, np.int32), "anchors4x4": np.zeros((mw, 4, 4)),
           "lambda": np.zeros(mw), "status": np.zeros(mw, np.int32)}
    ctx._chk(load().orbx_stitch_fetch(ctx._h, first_frame, nf, _ptr(out["trajectory4x4"]), _ptr(out["owner"]),
                                      first_window, nw, _ptr(out["anchors4x4"]), _ptr(out["lambda"]),
                                      _ptr(out["status"])))
    return {k: a[:nf if k in ("trajectory4x4", "owner") else nw] for k, a in out.items()}


def stitch_windows(poses, stride, T_start=None, align_scale=False):
    """orbx_stitch_windows: the join on the host, no context.  poses (n_windows, window_len, 4, 4): the dict of
    stitch_fetch."""
    if np.ndim(poses) != 4 or np.shape(poses)[2:] != (4, 4):
        raise ValueError("poses must be (n_windows, window_len, 4, 4)")
    poses = _f64(poses, np.shape(poses))
    n, L = poses.shape[:2]
    T_start = _t_start(T_start)
    F = max(stream_frames(n, L, stride), 1)
    out = {"trajectory4x4": np.zeros((F, 4, 4)), "owner": np.zeros(F, np.int32), "anchors4x4": np.zeros((max(n, 1), 4, 4)),
           "lambda": np.zeros(max(n, 1)), "status": np.zeros(max(n, 1), np.int32)}
    st = load().orbx_stitch_windows(_dp(poses), n, L, stride, None if T_start is None else _dp(T_start),
                                    int(bool(align_scale)), _ptr(out["trajectory4x4"]), _ptr(out["owner"]),
                                    _ptr(out["anchors4x4"]), _ptr(out["lambda"]), _ptr(out["status"]))
    if st != OK:
        raise OrbxError(st, "orbx_stitch_windows")
    return out


def stream_odometry_tracks_device(ctx, K, tracks, seen=None, stride=1, T_start=None, scale0_first=1.0, prob=0.999,
                                  threshold=1.0, pose_max_iters=1000, seed=0, tri_mode=orbx_lm.TRI_FIRST_TWO,
                                  max_reproj_px=0.0, huber_delta=1.0, ba_max_iters=200,
                                  max_rot=orbx_vo.MAX_ROT_DIFF, max_trans=orbx_vo.MAX_TRANS_DIFF, align_scale=False,
                                  n_windows=None, slot_capacity=None, window_len=None, stream=None):
    """orbx_stream_odometry_tracks_device: tracks pose, the stream's chain, landmarks, solve, write-back gate and
    stitch of a stream of overlapping windows, without a fetch.  The tracks arguments are those of
    Context.tracks_pose (an LkWindowsView, tensors, arrays or raw addresses).  Asynchronous; every stage's own fetch
    delivers its block, stitch_fetch the trajectory."""
    tracks, seen, n_windows, slot_capacity, window_len, ctx._st_tracks_keep = _tracks_args(
        tracks, seen, n_windows, slot_capacity, window_len)  # (the tensors: kept alive until the next call)
    K, T_start = _f64(K, (3, 3)), _t_start(T_start)
    ctx._chk(load().orbx_stream_odometry_tracks_device(
        ctx._h, _dp(K), tracks, seen, n_windows, slot_capacity, window_len, stride,
        None if T_start is None else _dp(T_start), scale0_first, prob, threshold, pose_max_iters, seed, tri_mode,
        max_reproj_px, huber_delta, ba_max_iters, max_rot, max_trans, int(bool(align_scale)), _stream(stream)))


def stream_odometry_tracks(ctx, K, tracks, seen, stride, T_start=None, scale0_first=1.0, prob=0.999, threshold=1.0,
                           pose_max_iters=1000, seed=0, tri_mode=orbx_lm.TRI_FIRST_TWO, max_reproj_px=0.0,
                           huber_delta=1.0, ba_max_iters=200, max_rot=orbx_vo.MAX_ROT_DIFF,
                           max_trans=orbx_vo.MAX_TRANS_DIFF, align_scale=False):
    """orbx_stream_odometry_tracks: host tracks (n_windows, slots, window_len, 2) and seen (n_windows, slots) from
    tracks pose to the trajectory.  Returns a dict of trajectory4x4 (F, 4, 4), st_status, wp_status, lm_status
    (n_windows,) and summaries (a list of dicts)."""
    tracks = np.ascontiguousarray(tracks, np.float32)
    if tracks.ndim != 4 or tracks.shape[3] != 2:
        raise ValueError("tracks must be (n_windows, slots, window_len, 2) float32")
    n, slots, wl = tracks.shape[:3]
    seen = np.ascontiguousarray(seen, np.int32).reshape(-1)
    if len(seen) != n * slots:
        raise ValueError("seen must have one entry per window and slot")
    K, T_start = _f64(K, (3, 3)), _t_start(T_start)
    m = max(n, 1)
    traj = np.zeros((max(stream_frames(n, wl, stride), 1), 4, 4))
    st_s, wp_s, lm_s = np.full(m, -1, np.int32), np.full(m, -1, np.int32), np.full(m, -1, np.int32)
    sums = (BaSummary * m)()
    ctx._chk(load().orbx_stream_odometry_tracks(
        ctx._h, _dp(K), _ptr(tracks), _ptr(seen), n, slots, wl, stride, None if T_start is None else _dp(T_start),
        scale0_first, prob, threshold, pose_max_iters, seed, tri_mode, max_reproj_px, huber_delta, ba_max_iters,
        max_rot, max_trans, int(bool(align_scale)), _dp(traj), _ptr(st_s), _ptr(wp_s), _ptr(lm_s), sums))
    return dict(trajectory4x4=traj, st_status=st_s[:n], wp_status=wp_s[:n], lm_status=lm_s[:n],
                summaries=[s.as_dict() for s in sums[:n]])
