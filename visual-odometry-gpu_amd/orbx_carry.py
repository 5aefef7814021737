"""ctypes binding of include/orbx_carry.h, the sixth public header of liborbx.so: landmarks
carried from the current landmarks block into the next generation of windows, the PnP of every frame of those windows
against them, the landmarks build from those poses and the one window of host arrays.  The functions take a Context of
`orbx`; the library is the one orbx.load() returns, and this module's own prototype table is applied to it once
(tests/test_orbx_carry_abi.py checks it against the header)."""
import ctypes as C

import numpy as np

from . import orbx
from .orbx import _count, _device_arg, _dp, _f64, _host_window, _i32, _ip, _ptr, _stream, _sync_uploads, _tracks_args
from .orbx_pnp import RECORD_DTYPE, _M64

CARRY_BUILT, CARRY_SOLVED = range(2)
CARRY_OK, CARRY_LOST = range(2)

P, I, D, U64 = orbx.P, orbx.I, orbx.D, orbx.U64
PROTOTYPES = {
    "orbx_landmarks_carry_device": (I, [P, P, I, I, I, P]),
    "orbx_landmarks_carry_results_device": (I, [P, P]),
    "orbx_landmarks_carry_fetch": (I, [P, I, I, P, P, P]),
    "orbx_window_poses_pnp_carried_device": (I, [P, P, P, P, I, I, I, D, D, I, U64, I, I, P]),
    "orbx_window_poses_pnp_carried_results_device": (I, [P, P]),
    "orbx_window_poses_pnp_carried_fetch": (I, [P, I, I, P, P, P]),
    "orbx_window_poses_pnp_carried_mask_fetch": (I, [P, I, I, P, I, P]),
    "orbx_landmarks_build_carried_device": (I, [P, P, P, P, I, I, I, P]),
    "orbx_localise_carried_window": (I, [P, P, P, I, P, P, P, I, I, P, D, D, I, U64, I, I, P, P, P, P]),
}
EXPORTS = list(PROTOTYPES)  # every symbol include/orbx_carry.h declares


class LandmarksCarryView(C.Structure):
    _fields_ = [("xyz", C.c_void_p), ("point", C.c_void_p), ("count", C.c_void_p), ("slot_capacity", C.c_int32),
                ("n_windows", C.c_int32)]


class WindowPosesCarriedView(C.Structure):
    _fields_ = [("records", C.c_void_p), ("poses6", C.c_void_p), ("mask", C.c_void_p), ("window_status", C.c_void_p),
                ("slot_capacity", C.c_int32), ("window_len", C.c_int32), ("n_windows", C.c_int32)]


_lib = None


def load():
    """The library of orbx.load() with every prototype of PROTOTYPES declared."""
    global _lib
    if _lib is None:
        lib = orbx.load()
        for name, (restype, argtypes) in PROTOTYPES.items():
            f = getattr(lib, name, None)  # (a symbol the library lacks is tests/test_orbx_carry_abi.py's to report)
            if f is not None:
                f.restype = restype
                f.argtypes = argtypes
        _lib = lib
    return _lib


def landmarks_carry(ctx, origin, n_windows=None, slot_capacity=None, source=CARRY_BUILT, stream=None):
    """orbx_landmarks_carry_device: joins origin (n_windows, slot_capacity) int32 -- a torch device tensor, a numpy
    array (copied to the device first) or a raw device address such as the top-up view's origin (then with both
    sizes) -- to the context's current landmarks block.  Asynchronous; landmarks_carry_fetch delivers the block."""
    keep = []
    origin, t, uploaded = _device_arg(origin, np.int32, lambda t: t.dim() == 2,
                                      "origin must be (n_windows, slot_capacity) int32, contiguous, on the device", keep)
    if t is None:
        if None in (n_windows, slot_capacity):
            raise ValueError("a raw origin address needs n_windows and slot_capacity")
    elif (n_windows, slot_capacity) not in ((None, None), tuple(t.shape)):
        raise ValueError("n_windows / slot_capacity differ from origin.shape")
    else:
        n_windows, slot_capacity = t.shape
    _sync_uploads(uploaded)
    ctx._carry_keep = keep  # (the tensor: kept alive until the next carry)
    ctx._chk(load().orbx_landmarks_carry_device(ctx._h, origin, n_windows, slot_capacity, source, _stream(stream)))


def landmarks_carry_view(ctx):
    """The device-side block of the last landmarks_carry (orbx_landmarks_carry_results_device)."""
    v = LandmarksCarryView()
    ctx._chk(load().orbx_landmarks_carry_results_device(ctx._h, C.byref(v)))
    return v


def landmarks_carry_fetch(ctx, first=0, n=None):
    """Windows [first, first + n) of the last landmarks_carry: a dict of xyz (n, slot_capacity, 3), point
    (n, slot_capacity) int32 and count (n) int32."""
    v = landmarks_carry_view(ctx)
    n = _count(n, first, v.n_windows)
    m = max(n, 1)
    xyz, point = np.zeros((m, v.slot_capacity, 3)), np.zeros((m, v.slot_capacity), np.int32)
    count = np.zeros(m, np.int32)
    ctx._chk(load().orbx_landmarks_carry_fetch(ctx._h, first, n, _ptr(xyz), _ptr(point), _ptr(count)))
    return dict(xyz=xyz[:n], point=point[:n], count=count[:n])


def window_poses_pnp_carried(ctx, K, tracks, seen, n_windows=None, slot_capacity=None, window_len=None, prob=0.99,
                             threshold_px=2.0, max_iters=1000, seed=0, refine_iters=10, min_inliers=4, stream=None):
    """orbx_window_poses_pnp_carried_device: every (window, frame) of the new windows' tracks -- the arguments of
    Context.landmarks_build -- against the last carry block.  Asynchronous; window_poses_pnp_carried_fetch delivers
    the results."""
    tracks, seen, n_windows, slot_capacity, window_len, ctx._carried_keep = _tracks_args(
        tracks, seen, n_windows, slot_capacity, window_len)
    K = _f64(K, (3, 3))
    ctx._chk(load().orbx_window_poses_pnp_carried_device(ctx._h, _dp(K), tracks, seen, n_windows, slot_capacity,
                                                         window_len, prob, threshold_px, max_iters, seed & _M64,
                                                         refine_iters, min_inliers, _stream(stream)))


def window_poses_pnp_carried_view(ctx):
    """The device-side block of the last window_poses_pnp_carried (orbx_window_poses_pnp_carried_results_device)."""
    v = WindowPosesCarriedView()
    ctx._chk(load().orbx_window_poses_pnp_carried_results_device(ctx._h, C.byref(v)))
    return v


def window_poses_pnp_carried_fetch(ctx, first=0, n=None, masks=True):
    """Windows [first, first + n) of the last window_poses_pnp_carried: a dict of records (n, window_len) in
    orbx_pnp.RECORD_DTYPE, poses6 (n, window_len, 6), window_status (n) int32 and, with masks, mask
    (n, window_len, slot_capacity) uint8, indexed by slot."""
    v = window_poses_pnp_carried_view(ctx)
    n = _count(n, first, v.n_windows)
    m = max(n, 1)
    rec, poses = np.zeros((m, v.window_len), RECORD_DTYPE), np.zeros((m, v.window_len, 6))
    status = np.zeros(m, np.int32)
    ctx._chk(load().orbx_window_poses_pnp_carried_fetch(ctx._h, first, n, _ptr(rec), _ptr(poses), _ptr(status)))
    out = dict(records=rec[:n], poses6=poses[:n], window_status=status[:n])
    if masks:
        out["mask"] = np.stack([np.stack([window_poses_pnp_carried_mask(ctx, first + w, k, v.slot_capacity)
                                          for k in range(v.window_len)]) for w in range(n)])
    return out


def window_poses_pnp_carried_mask(ctx, window, k, capacity=None):
    """orbx_window_poses_pnp_carried_mask_fetch: the mask of problem (window, k), one byte per slot."""
    if capacity is None:
        capacity = window_poses_pnp_carried_view(ctx).slot_capacity
    mask, cnt = np.zeros(max(capacity, 1), np.uint8), C.c_int(0)
    ctx._chk(load().orbx_window_poses_pnp_carried_mask_fetch(ctx._h, window, k, _ptr(mask), capacity, C.byref(cnt)))
    return mask[:cnt.value].copy()


def landmarks_build_carried(ctx, K, tracks, seen, n_windows=None, slot_capacity=None, window_len=None, stream=None):
    """orbx_landmarks_build_carried_device: Context.landmarks_build with the poses read from the last
    window_poses_pnp_carried on the device.  Asynchronous; Context.landmarks_fetch delivers the block."""
    tracks, seen, n_windows, slot_capacity, window_len, ctx._lm_keep = _tracks_args(
        tracks, seen, n_windows, slot_capacity, window_len)
    K = _f64(K, (3, 3))
    ctx._chk(load().orbx_landmarks_build_carried_device(ctx._h, _dp(K), tracks, seen, n_windows, slot_capacity,
                                                        window_len, _stream(stream)))


def localise_carried_window(ctx, old_points3, old_slot_of_point, origin, tracks, seen, K, prob=0.99, threshold_px=2.0,
                            max_iters=1000, seed=0, refine_iters=10, min_inliers=4):
    """orbx_localise_carried_window: one window of host arrays.  old_points3 (n_old, 3) and old_slot_of_point (n_old)
    are an old window's landmarks; origin and seen (slots) and tracks (slots, window_len, 2) are the new window.
    Returns a dict of records (window_len), poses6 (window_len, 6), window_status and carried_point (slots)."""
    tracks, seen, slots, wl = _host_window(tracks, seen)
    pts, sop, origin, K = _f64(old_points3, (-1, 3)), _i32(old_slot_of_point), _i32(origin), _f64(K, (3, 3))
    if len(pts) != len(sop) or len(origin) != slots:
        raise ValueError("old_points3 / old_slot_of_point or origin / seen differ in length")
    n_old = len(pts)
    rec, poses = np.zeros(max(wl, 1), RECORD_DTYPE), np.zeros((max(wl, 1), 6))
    status, point = C.c_int32(-1), np.zeros(max(slots, 1), np.int32)
    ctx._chk(load().orbx_localise_carried_window(ctx._h, _dp(pts) if n_old else None, _ip(sop) if n_old else None,
                                                 n_old, _ip(origin), _ptr(tracks), _ptr(seen), slots, wl, _dp(K),
                                                 prob, threshold_px, max_iters, seed & _M64, refine_iters,
                                                 min_inliers, _ptr(rec), _ptr(poses), C.byref(status), _ptr(point)))
    return dict(records=rec[:wl], poses6=poses[:wl], window_status=status.value, carried_point=point[:slots])
