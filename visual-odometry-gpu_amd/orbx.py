"""ctypes binding of liborbx.so (include/orbx.h) for tests and bench.py.

The product is the C-ABI library; this module is only the thinnest possible
Python view of it (numpy arrays in / out, device pointers as ints).  It never
falls back to a CPU implementation: if liborbx.so is missing or no gfx950
device is present, loading / Context creation raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ORBX_LIB") or os.path.join(_HERE, "liborbx.so")  # ORBX_LIB: A/B builds (diagnostics)

MAX_LEVELS = 16
OK, ERR_INVALID_ARG, ERR_CAPACITY, ERR_HIP, ERR_NO_DEVICE, ERR_UNSUPPORTED = range(6)
SELECT_HARRIS, SELECT_ROWMAJOR = 0, 1
BLUR_NONE, BLUR_UPPER, BLUR_ALL = 0, 1, 2
BLUR_SEP16, BLUR_K273 = 0, 1
STAGE_PYRAMID, STAGE_BLUR, STAGE_FAST, STAGE_COMPACT, STAGE_HARRIS, STAGE_SELECT, STAGE_DESCRIBE = range(7)
NUM_STAGE_TIMES = 8
STAGE_NAMES = ["pyramid", "blur", "fast_nms", "compact", "harris", "select", "describe", "total"]
POSE_MAX_ITERS = 100000  # ORBX_POSE_MAX_ITERS
BA_CONVERGENCE, BA_NO_CONVERGENCE, BA_FAILURE, BA_SKIPPED = range(4)
BA_MAX_POSES = 8
LK_FB_ALIVE, LK_FB_FORWARD, LK_FB_BACKWARD, LK_FB_DISTANCE = range(4)  # `lost` of the forward-backward check
LM_OK, LM_BASELINE, LM_EMPTY, LM_BAD_POSE = range(4)

# ---- the prototype of every function include/orbx.h declares: name -> (return type, parameter types), applied once
# by load() (tests/test_binding_prototypes.py checks it against the header).  Every pointer, the handle included, is
# a c_void_p: it takes an array's address, a device address, byref(..), a typed pointer or None alike.
P, I, Z, D, F, U64 = C.c_void_p, C.c_int, C.c_size_t, C.c_double, C.c_float, C.c_uint64
_IMAGE = [P, P, I, I, I]  # ctx, image, width, height, stride
_FRAMES = [P, P, I, I, I, I, Z]  # ctx, frames, n, width, height, row_stride, frame_stride
_LK = [I, I, I, D]  # win_size, max_level, max_iters, epsilon
_LK_WINDOWS = _FRAMES + [P, I, I, P, P, I] + _LK  # .. window_first, n_windows, window_len, points, counts, slots ..
_LK_WINDOW = _FRAMES + [P, I, P, P, P] + _LK  # .. pts, n, tracks, seen, err ..
_BATCH_FETCH = [P, I, I] + [P] * 7 + [I]
PROTOTYPES = {
    # context, whole path, switches and diagnostics
    "orbx_params_default_gpu": (I, [P]), "orbx_params_default_cpu": (I, [P]), "orbx_create": (I, [P, P]),
    "orbx_destroy": (None, [P]), "orbx_last_error_string": (C.c_char_p, [P]), "orbx_status_string": (C.c_char_p, [I]),
    "orbx_version": (C.c_char_p, []), "orbx_get_plan": (I, [P, I, I] + [P] * 6),
    "orbx_detect_and_compute": (I, _IMAGE + [P] * 6 + [I, P]),
    "orbx_detect_and_compute_batch_device": (I, _FRAMES + [P]), "orbx_detect_and_compute_batch_host": (I, _FRAMES),
    "orbx_wait": (I, [P]), "orbx_batch_results_device": (I, [P, P]), "orbx_batch_results_host": (I, [P, I, P]),
    "orbx_batch_fetch": (I, _BATCH_FETCH), "orbx_batch_fetch_previous": (I, _BATCH_FETCH),
    "orbx_batch_prefetch": (I, [P]), "orbx_batch_prefetch_compact": (I, [P]),
    "orbx_enable_stage_timing": (I, [P, I]), "orbx_last_stage_times": (I, [P, P]),
    "orbx_stage_times_history": (I, [P, I, P]), "orbx_bench_stage": (I, [P, I, I, I, P]),
    "orbx_set_fast_early_exit": (I, [P, I]), "orbx_set_fused_pyramid_blur": (I, [P, I]),
    "orbx_set_top_rows_first": (I, [P, I]), "orbx_set_pipelined_batches": (I, [P, I]),
    "orbx_set_host_results": (I, [P, I]), "orbx_fast_tile_counts": (I, [P, P, P]),
    "orbx_pyramid_pixel_counts": (I, [P, P, P]), "orbx_debug_fill_pools": (I, [P, I]),
    "orbx_debug_read_pyramid_level": (I, [P, I, I, P, Z]),
    "orbx_lk_track": (I, [P, P, I, P, I, I, I, P, I, P, P, P] + _LK), "orbx_lk_pyramid_levels": (I, [I] * 4),
    # stage operators
    "orbx_fast_score": (I, _IMAGE + [I, I, P]), "orbx_nms": (I, [P, P, I, I, I, I, F, P, P, P]),
    "orbx_fast": (I, _IMAGE + [I, I, I, I, P, P, P]), "orbx_orientations": (I, _IMAGE + [P, I, I, P]),
    "orbx_brief": (I, _IMAGE + [P, P, I, P]), "orbx_harris": (I, _IMAGE + [P, I, I, F, P]),
    "orbx_blur5_sep": (I, _IMAGE + [P, I]), "orbx_blur5_273": (I, _IMAGE + [P, I]),
    "orbx_conv2d": (I, _IMAGE + [P, I, P]), "orbx_gaussian_blur_conv": (I, _IMAGE + [I, P]),
    "orbx_gaussian_kernel": (I, [I, F, P]), "orbx_sobel": (I, _IMAGE + [I, P]),
    "orbx_build_pyramid_level": (I, _IMAGE + [I, P, P, P]), "orbx_select_top": (I, [P, P, I, I, P, P]),
    # matcher, pose, scale, bundle adjustment
    "orbx_knn2": (I, [P, P, I, P, I, P, P]), "orbx_match_ratio": (I, [P, P, I, P, I, D, P, P, P, I, P]),
    "orbx_batch_match_consecutive": (I, [P, D]), "orbx_batch_match_fetch": (I, [P, I, P, P, P, I, P]),
    "orbx_estimate_pose": (I, [P, P, P, I, P, D, D, I, U64] + [P] * 7),
    "orbx_batch_pose_consecutive": (I, [P, P, D, D, I, U64]), "orbx_batch_pose_fetch": (I, [P, I, I] + [P] * 6),
    "orbx_batch_pose_mask": (I, [P, I, P, I, P]), "orbx_triangulate": (I, [P, P, P, I] + [P] * 5),
    "orbx_estimate_scale": (I, [P, P, P, I, P, P, I, P, P]), "orbx_batch_scale_consecutive": (I, [P, P]),
    "orbx_batch_scale_fetch": (I, [P, I, I, P, P, P]), "orbx_batch_points_fetch": (I, [P, I, P, P, I, P]),
    "orbx_chain_trajectory": (I, [P, P, P, P, I, P]),
    "orbx_bundle_adjust": (I, [P, P, I, P, I, P, I, P, P, P, D, I, P]),
    "orbx_bundle_adjust_batch": (I, [P, P, I] + [P] * 8 + [D, I, P]),
    # good features and their top-up
    "orbx_corner_min_eigen_val": (I, _IMAGE + [P]), "orbx_good_features_to_track": (I, _IMAGE + [I, D, D, P, I, P]),
    "orbx_good_features_batch_device": (I, _FRAMES + [I, D, D, P]),
    "orbx_good_features_workspace_limit": (I, [P, Z]), "orbx_good_features_results_device": (I, [P, P]),
    "orbx_good_features_fetch": (I, [P, I, I, P, P]),
    "orbx_good_features_topup_device": (I, _FRAMES + [P, Z, Z, P, I, I, I, D, D, P]),
    "orbx_good_features_topup_results_device": (I, [P, P]), "orbx_good_features_topup_fetch": (I, [P, I, I] + [P] * 4),
    "orbx_good_features_topup": (I, _IMAGE + [P, I, I, D, D, P, P, I, P, P]),
    "orbx_good_features_to_track_masked": (I, _IMAGE + [P, I, I, D, D, P, I, P]),
    # Lucas-Kanade over frame windows
    "orbx_lk_track_windows_device": (I, _LK_WINDOWS + [P]),
    "orbx_lk_track_windows_fb_device": (I, _LK_WINDOWS + [F, P]),
    "orbx_lk_windows_results_device": (I, [P, P]), "orbx_lk_windows_fb_results_device": (I, [P, P]),
    "orbx_lk_windows_fetch": (I, [P, I, I, P, P, P]), "orbx_lk_windows_fb_fetch": (I, [P, I, I, P, P]),
    "orbx_lk_workspace_limit": (I, [P, Z]), "orbx_lk_track_window": (I, _LK_WINDOW),
    "orbx_lk_track_window_fb": (I, _LK_WINDOW + [F, P, P]),
    # landmarks, their bundle adjustment, pose and scale of tracked pairs
    "orbx_landmarks_build_device": (I, [P, P, P, P, I, I, I, P, P]), "orbx_landmarks_results_device": (I, [P, P]),
    "orbx_landmarks_fetch": (I, [P, I, I] + [P] * 6 + [I] + [P] * 3 + [I, P, P]),
    "orbx_bundle_adjust_landmarks_device": (I, [P, D, I, P]),
    "orbx_bundle_adjust_landmarks_fetch": (I, [P, I, I, P, P, P, I, P]),
    "orbx_bundle_adjust_tracks": (I, [P, P, P, P, I, I, P, D, I, P, P, P, P, I, P]),
    "orbx_tracks_pose_device": (I, [P, P, P, P, I, I, I, D, D, I, U64, P]),
    "orbx_tracks_pose_results_device": (I, [P, P]), "orbx_tracks_pose_fetch": (I, [P, I, I] + [P] * 10),
    "orbx_tracks_pose_pair_fetch": (I, [P, I] + [P] * 4 + [I, P]),
    "orbx_tracks_pose": (I, [P, P, P, P, I, I, D, D, I, U64] + [P] * 10),
}
EXPORTS = list(PROTOTYPES)  # every symbol include/orbx.h declares (checked by tests/test_abi.py)


class Params(C.Structure):
    _fields_ = [
        ("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32),
        ("threshold", C.c_int32), ("n", C.c_int32), ("nms_window", C.c_int32), ("patch_size", C.c_int32),
        ("harris_window", C.c_int32), ("harris_k", C.c_float), ("select_mode", C.c_int32),
        ("blur_levels", C.c_int32), ("blur_kind", C.c_int32), ("max_width", C.c_int32),
        ("max_height", C.c_int32), ("max_batch", C.c_int32), ("device", C.c_int32),
    ]


class BatchView(C.Structure):
    _fields_ = [
        ("counts", C.c_void_p), ("keypoints", C.c_void_p), ("level_kps", C.c_void_p),
        ("orientations", C.c_void_p), ("responses", C.c_void_p), ("levels", C.c_void_p),
        ("descriptors", C.c_void_p), ("slot_capacity", C.c_int32), ("n", C.c_int32),
        ("keypoints16", C.c_void_p),
    ]


class BaSummary(C.Structure):
    _fields_ = [("termination", C.c_int32), ("iterations", C.c_int32), ("successful_steps", C.c_int32),
                ("reserved", C.c_int32), ("initial_cost", C.c_double), ("final_cost", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k in ("termination", "iterations", "successful_steps", "initial_cost",
                                              "final_cost")}


class GoodFeaturesView(C.Structure):
    _fields_ = [("counts", C.c_void_p), ("corners_xy", C.c_void_p), ("slot_capacity", C.c_int32), ("n", C.c_int32)]


class GoodFeaturesTopupView(C.Structure):
    _fields_ = [("counts", C.c_void_p), ("carried", C.c_void_p), ("points_xy", C.c_void_p), ("origin", C.c_void_p),
                ("slot_capacity", C.c_int32), ("n", C.c_int32)]


class LkWindowsView(C.Structure):
    _fields_ = [("tracks_xy", C.c_void_p), ("seen", C.c_void_p), ("err", C.c_void_p), ("slot_capacity", C.c_int32),
                ("window_len", C.c_int32), ("n_windows", C.c_int32)]


class LkWindowsFbView(C.Structure):
    _fields_ = [("fb_d2", C.c_void_p), ("lost", C.c_void_p), ("slot_capacity", C.c_int32), ("window_len", C.c_int32),
                ("n_windows", C.c_int32)]


class LandmarksView(C.Structure):
    _fields_ = [("status", C.c_void_p), ("pose_offset", C.c_void_p), ("point_offset", C.c_void_p),
                ("obs_offset", C.c_void_p), ("points3", C.c_void_p), ("rows", C.c_void_p), ("obs_pose", C.c_void_p),
                ("obs_xy", C.c_void_p), ("slot_of_point", C.c_void_p), ("slot_capacity", C.c_int32),
                ("window_len", C.c_int32), ("n_windows", C.c_int32)]


class TracksPoseView(C.Structure):
    _fields_ = [("pose", C.c_void_p), ("n", C.c_void_p), ("scale", C.c_void_p), ("slot_of", C.c_void_p),
                ("mask", C.c_void_p), ("xyz", C.c_void_p), ("valid", C.c_void_p), ("slot_capacity", C.c_int32),
                ("window_len", C.c_int32), ("n_windows", C.c_int32), ("n_pairs", C.c_int32)]


class OrbxError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("liborbx status %d (%s): %s" % (status, _status_string(status), msg))
        self.status = status


_lib = None


def _share_hip_runtime_with_torch():
    """PyTorch-ROCm wheels bundle their own libamdhip64/libhsa-runtime64.  Two HIP
    runtimes in one process cannot both open the GPU, so when torch is installed
    pre-load ITS runtime (same soname, libamdhip64.so.7) before liborbx.so; the
    dynamic loader then binds liborbx's NEEDED entry to it.  Without torch, or
    with ORBX_HIP_RUNTIME=system, liborbx uses /opt/rocm's runtime."""
    if os.environ.get("ORBX_HIP_RUNTIME", "torch") != "torch":
        return
    try:
        import importlib.util

        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass


def load():
    """Load liborbx.so (raises OSError if it has not been built) and declare every prototype of PROTOTYPES."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError("liborbx.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `make -C visual-odometry-gpu_amd/csrc` (there is no CPU fallback)")
        _share_hip_runtime_with_torch()
        lib = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in PROTOTYPES.items():
            f = getattr(lib, name, None)  # (a symbol the library lacks is build()'s and tests/test_abi.py's to report)
            if f is not None:
                f.restype = restype
                f.argtypes = argtypes
        _lib = lib
    return _lib


def _status_string(st):
    try:
        return load().orbx_status_string(int(st)).decode()
    except OSError:
        return "?"


def default_params(flavour="gpu", **kw):
    """orbx_params with the reference defaults of the GPU (orb.hpp) or CPU (orb_cpu.hpp) flavour."""
    p = Params()
    fn = load().orbx_params_default_gpu if flavour == "gpu" else load().orbx_params_default_cpu
    fn(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


# ---- host arguments
def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _img(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.ndim != 2:
        raise ValueError("image must be 2-D uint8")
    return a


def _gftt_view(a):
    # a row-strided uint8 view (a region of a larger image) is handed over as it is
    if isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.ndim == 2 and a.strides[1] == 1 and \
            a.strides[0] >= a.shape[1]:
        return a
    return _img(a)


def _kps(k):
    return np.ascontiguousarray(k, dtype=np.int32).reshape(-1, 2)


def _desc(d):
    return np.ascontiguousarray(d, dtype=np.uint8).reshape(-1, 32)


def _f64(a, shape, copy=False):
    """`a` as a C-contiguous float64 array of `shape` (K: (3, 3)) for _dp(); copy: always one of the binding's own,
    for an entry that writes in place."""
    a = np.asarray(a, np.float64).reshape(shape)
    return np.array(a, order="C") if copy else np.ascontiguousarray(a)


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1))


# The arrays of _f64 and _i32 go to the library as typed pointers, which every prototype a caller may have put on the
# shared function object takes: the table's c_void_p, and a POINTER(c_double) / POINTER(c_int32) of the caller's own.
def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _point_pairs(pts1, pts2):
    p1 = np.ascontiguousarray(np.asarray(pts1, np.float32).reshape(-1, 2))
    p2 = np.ascontiguousarray(np.asarray(pts2, np.float32).reshape(-1, 2))
    if p1.shape != p2.shape:
        raise ValueError("pts1 and pts2 differ in shape")
    return p1, p2, p1.shape[0]


def _observations(obs_point, obs_pose, obs_xy):
    op, oq, xy = _i32(obs_point), _i32(obs_pose), _f64(obs_xy, (-1, 2), copy=True)
    if not len(op) == len(oq) == len(xy):
        raise ValueError("obs_point, obs_pose and obs_xy differ in length")
    return op, oq, xy


def _host_window(tracks, seen):
    """One window of host tracks (slots, window_len, 2) and seen (slots): (tracks, seen, slots, window_len)."""
    tracks = np.ascontiguousarray(tracks, np.float32)
    if tracks.ndim != 3 or tracks.shape[2] != 2:
        raise ValueError("tracks must be (slots, window_len, 2) float32")
    seen = np.ascontiguousarray(seen, np.int32).reshape(-1)
    if len(seen) != tracks.shape[0]:
        raise ValueError("seen must have one entry per slot")
    return (tracks, seen) + tracks.shape[:2]


def _stream(stream):
    """A hipStream_t given as an int, or None / 0 for the context's own stream."""
    return stream or None


def _count(n, first, total):
    """The n of a fetch of [first, first + n); None: everything from `first` on.  total: a number, or a call that
    yields it (made only then)."""
    if n is not None:
        return n
    return (total() if callable(total) else total) - first


# ---- device arguments (free of Context: tests/test_binding_prototypes.py runs their refusals without a GPU)
def _frame_strides(shape, strides):
    """(row_stride, frame_stride) of an (n, h, w) batch with these strides.  One frame may come with any stride(0)
    -- 0 after expand(), the batch's own after a slice -- so it gets at least the frame's own extent."""
    n, h, w = shape
    rs = strides[1]
    return rs, max(strides[0], rs * (h - 1) + w) if n == 1 else strides[0]


def _frames_arg(frames):
    """An (n, h, w) uint8 frames argument, a torch device tensor (any strides with unit pixel stride) or a numpy array
    (copied to the device): (tensor, n, h, w, row_stride, frame_stride, whether it was uploaded)."""
    import torch

    uploaded = isinstance(frames, np.ndarray)
    if uploaded:
        frames = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.uint8)).cuda()
    if frames.dtype != torch.uint8 or frames.dim() != 3 or not frames.is_cuda or frames.stride(2) != 1:
        raise ValueError("frames must be (n, h, w) uint8 on the device with unit pixel stride")
    return (frames,) + tuple(frames.shape) + _frame_strides(frames.shape, frames.stride()) + (uploaded,)


def _device_arg(a, dtype, shape_ok, message, keep):
    """A device array given as a contiguous torch device tensor of `dtype` (checked with shape_ok(tensor), refused
    with `message`, appended to `keep`), as a numpy array (copied to the device first) or as a raw device address
    or None (passed through): (address, the tensor or None, whether it was uploaded)."""
    import torch

    uploaded = isinstance(a, np.ndarray)
    if uploaded:
        a = torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()
    if not torch.is_tensor(a):
        return a, None, False
    if a.dtype != getattr(torch, np.dtype(dtype).name) or not a.is_cuda or not a.is_contiguous() or not shape_ok(a):
        raise ValueError(message)
    keep.append(a)
    return a.data_ptr(), a, uploaded


def _sync_uploads(*uploaded):
    if any(uploaded):
        import torch

        torch.cuda.synchronize()  # the uploads ran on torch's stream


def _lk_points_arg(points, n_windows, slot_capacity, keep):
    """The points of lk_track_windows: (address, slot_capacity, whether they were uploaded)."""
    points, t, uploaded = _device_arg(
        points, np.float32, lambda t: t.dim() == 3 and t.shape[0] == n_windows and t.shape[2] == 2,
        "points must be (n_windows, slot_capacity, 2) float32, contiguous, on the device", keep)
    if t is None:
        if slot_capacity is None:
            raise ValueError("a raw points address needs slot_capacity")
    elif slot_capacity not in (None, t.shape[1]):
        raise ValueError("slot_capacity differs from points.shape[1]")
    else:
        slot_capacity = t.shape[1]
    return points, slot_capacity, uploaded


def _tracks_args(tracks, seen, n_windows, slot_capacity, window_len):
    """The tracks block of landmarks_build and tracks_pose: an LkWindowsView (seen and the three sizes come from it),
    or tracks and seen as torch device tensors, numpy arrays (copied to the device, and waited for) or raw device
    addresses (then with the three sizes): (tracks address, seen address, n_windows, slot_capacity, window_len, the
    tensors to keep alive)."""
    if isinstance(tracks, LkWindowsView):
        v = tracks
        tracks, seen = v.tracks_xy, v.seen
        n_windows, slot_capacity, window_len = v.n_windows, v.slot_capacity, v.window_len
    keep = []
    tracks, t, up_tracks = _device_arg(
        tracks, np.float32, lambda t: t.dim() == 4 and t.shape[3] == 2,
        "tracks must be (n_windows, slots, window_len, 2) float32, contiguous, on the device", keep)
    if t is None:
        if None in (n_windows, slot_capacity, window_len):
            raise ValueError("a raw tracks address needs n_windows, slot_capacity and window_len")
    elif (n_windows, slot_capacity, window_len) not in ((None, None, None), tuple(t.shape[:3])):
        raise ValueError("n_windows / slot_capacity / window_len differ from tracks.shape")
    else:
        n_windows, slot_capacity, window_len = t.shape[:3]
    seen, _, up_seen = _device_arg(seen, np.int32, lambda t: t.numel() == n_windows * slot_capacity,
                                   "seen must be (n_windows, slots) int32, contiguous, on the device", keep)
    _sync_uploads(up_tracks, up_seen)
    return tracks, seen, n_windows, slot_capacity, window_len, keep


class _Core:
    """The context itself, the whole path and the stage operators."""

    def __init__(self, params=None, **kw):
        self._lib = load()
        if params is None:
            params = default_params(kw.pop("flavour", "gpu"), **kw)
        self.params = params
        h = C.c_void_p()
        st = self._lib.orbx_create(C.byref(params), C.byref(h))
        if st != OK:
            raise OrbxError(st, self._lib.orbx_last_error_string(None).decode())
        self._h = h
        self._cap_cache = {}
        self._dac = self._lib.orbx_detect_and_compute

    def close(self):
        if getattr(self, "_h", None):
            self._lib.orbx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, st, allow=()):
        if st != OK and st not in allow:
            raise OrbxError(st, self._lib.orbx_last_error_string(self._h).decode())
        return st

    # ---- geometry
    def plan(self, width, height):
        nl = self.params.nlevels
        lw = np.zeros(nl, np.int32)
        lh = np.zeros(nl, np.int32)
        q = np.zeros(nl, np.int32)
        cap = np.zeros(nl, np.int32)
        sc = np.zeros(nl, np.float32)
        oc = C.c_int32(0)
        self._chk(self._lib.orbx_get_plan(self._h, width, height, _ptr(lw), _ptr(lh), _ptr(q), _ptr(cap), _ptr(sc),
                                          C.byref(oc)))
        return dict(level_w=lw, level_h=lh, quota=q, fast_cap=cap, scale=sc, out_capacity=oc.value)

    # ---- whole path
    def detect_and_compute(self, image, capacity=None):
        """ORB::detectAndCompute (orb.hpp:37). Returns dict of numpy arrays."""
        image = _img(image)
        h, w = image.shape
        if capacity is None:
            capacity = self._cap_cache.get((w, h))
            if capacity is None:
                capacity = self._cap_cache[(w, h)] = max(self.plan(w, h)["out_capacity"], 1)
        kps = np.empty((capacity, 2), np.int32)
        lkp = np.empty((capacity, 2), np.int32)
        ang = np.empty(capacity, np.float32)
        resp = np.empty(capacity, np.float32)
        lev = np.empty(capacity, np.int32)
        desc = np.empty((capacity, 32), np.uint8)
        cnt = C.c_int(0)
        st = self._dac(self._h, image.ctypes.data, w, h, image.strides[0], kps.ctypes.data, ang.ctypes.data,
                       desc.ctypes.data, resp.ctypes.data, lev.ctypes.data, lkp.ctypes.data, capacity, C.byref(cnt))
        if st != OK and st != ERR_CAPACITY:
            self._chk(st)
        c = min(cnt.value, capacity)
        return dict(count=cnt.value, status=st, kps=kps[:c], kps_level=lkp[:c], angles=ang[:c], responses=resp[:c],
                    levels=lev[:c], desc=desc[:c])

    def batch_device(self, d_ptr, n, width, height, row_stride=None, frame_stride=None, stream=None):
        row_stride = width if row_stride is None else row_stride
        frame_stride = row_stride * height if frame_stride is None else frame_stride
        self._chk(self._lib.orbx_detect_and_compute_batch_device(self._h, d_ptr, n, width, height, row_stride,
                                                                 frame_stride, _stream(stream)))

    def batch_host(self, frames):
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if frames.ndim != 3:
            raise ValueError("frames must be (n, h, w) uint8")
        n, h, w = frames.shape
        self._chk(self._lib.orbx_detect_and_compute_batch_host(self._h, _ptr(frames), n, w, h, w, w * h))

    def wait(self):
        self._chk(self._lib.orbx_wait(self._h))

    def batch_view(self):
        v = BatchView()
        self._chk(self._lib.orbx_batch_results_device(self._h, C.byref(v)))
        return v

    def batch_host_view(self, previous=False):
        """Zero-copy numpy views of the pinned host mirror of a result block (orbx_batch_results_host); previous: how
        many batches back (False / 0: the last one, True / 1: the one before, up to 3)."""
        v = BatchView()
        self._chk(self._lib.orbx_batch_results_host(self._h, int(previous), C.byref(v)))
        n, cap = v.n, v.slot_capacity

        def arr(ptr, dtype, shape):
            if not ptr:  # (a section a compact prefetch did not copy)
                return None
            size = int(np.prod(shape)) * np.dtype(dtype).itemsize
            return np.frombuffer((C.c_char * size).from_address(ptr), dtype=dtype).reshape(shape)

        # kps16: the level-0 coordinates as (x, y) uint16 pairs (x | y << 16, little endian); the only keypoint
        # section of a compact copy
        return dict(counts=arr(v.counts, np.int32, (n,)), kps=arr(v.keypoints, np.int32, (n, cap, 2)),
                    kps16=arr(v.keypoints16, np.uint16, (n, cap, 2)),
                    kps_level=arr(v.level_kps, np.int32, (n, cap, 2)), angles=arr(v.orientations, np.float32, (n, cap)),
                    responses=arr(v.responses, np.float32, (n, cap)), levels=arr(v.levels, np.int32, (n, cap)),
                    desc=arr(v.descriptors, np.uint8, (n, cap, 32)))

    def batch_prefetch(self, compact=False):
        """Start the asynchronous D2H copy of the last batch's result block (overlaps the next batch); compact: only
        counts, packed keypoints (kps16), orientations and descriptors (orbx_batch_prefetch_compact)."""
        if compact:
            self._chk(self._lib.orbx_batch_prefetch_compact(self._h))
        else:
            self._chk(self._lib.orbx_batch_prefetch(self._h))

    def batch_fetch(self, first, n, capacity, previous=False):
        """Results of the last batch (previous=True: of the batch before it, see orbx_batch_fetch_previous)."""
        counts = np.zeros(n, np.int32)
        kps = np.zeros((n, capacity, 2), np.int32)
        lkp = np.zeros((n, capacity, 2), np.int32)
        ang = np.zeros((n, capacity), np.float32)
        resp = np.zeros((n, capacity), np.float32)
        lev = np.zeros((n, capacity), np.int32)
        desc = np.zeros((n, capacity, 32), np.uint8)
        fn = self._lib.orbx_batch_fetch_previous if previous else self._lib.orbx_batch_fetch
        st = fn(self._h, first, n, _ptr(counts), _ptr(kps), _ptr(ang), _ptr(desc), _ptr(resp), _ptr(lev), _ptr(lkp),
                capacity)
        self._chk(st, allow=(ERR_CAPACITY,))
        return dict(counts=counts, kps=kps, kps_level=lkp, angles=ang, responses=resp, levels=lev, desc=desc,
                    status=st)

    def enable_stage_timing(self, mode=1):
        """0/False off, 1/True events around every stage, 2 only around blur and fast+nms."""
        self._chk(self._lib.orbx_enable_stage_timing(self._h, int(mode)))

    def set_fast_early_exit(self, on=True):
        self._chk(self._lib.orbx_set_fast_early_exit(self._h, 1 if on else 0))

    def set_fused_pyramid_blur(self, on=True):
        self._chk(self._lib.orbx_set_fused_pyramid_blur(self._h, 1 if on else 0))

    def set_host_results(self, on=True):
        """The describe kernel also writes the compact record into the pinned host mirror (orbx_set_host_results)."""
        self._chk(self._lib.orbx_set_host_results(self._h, 1 if on else 0))

    def set_pipelined_batches(self, on=True):
        """Consecutive batch_device calls alternate between two lanes (own stream, own pools) and overlap."""
        self._chk(self._lib.orbx_set_pipelined_batches(self._h, 1 if on else 0))

    def set_top_rows_first(self, mode=2):
        """0: one pass, 1: the pyramid top rows first whenever eligible, 2: adaptive (default)."""
        self._chk(self._lib.orbx_set_top_rows_first(self._h, int(mode)))

    def debug_fill_pools(self, byte):
        """DEBUG (tests): fill the working pools of both lanes with `byte` (orbx_debug_fill_pools)."""
        self._chk(self._lib.orbx_debug_fill_pools(self._h, int(byte)))

    def debug_read_pyramid_level(self, frame, level, width, height):
        """DEBUG (tests): level `level` of frame `frame` of the current lane's blurred pyramid, as left by the last
        whole-path batch of width x height frames (orbx_debug_read_pyramid_level)."""
        plan = self.plan(width, height)
        out = np.zeros((int(plan["level_h"][level]), int(plan["level_w"][level])), np.uint8)
        self._chk(self._lib.orbx_debug_read_pyramid_level(self._h, int(frame), int(level), _ptr(out), out.size))
        return out

    def lk_track(self, prev, nxt, pts, win=21, max_level=3, max_iters=30, epsilon=0.01):
        """cv::calcOpticalFlowPyrLK(prev, next, pts, ...) as called at feature_tracking.cpp:175-181.
        prev=None: the previous call's `next` image is this call's `prev`.  Returns next_pts, status, err."""
        nxt = _img(nxt)
        h, w = nxt.shape
        if prev is not None:
            prev = _img(prev)
            if prev.shape != nxt.shape:
                raise ValueError("prev and next must have the same size")
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        n = len(pts)
        out = np.zeros((max(n, 1), 2), np.float32)
        st = np.zeros(max(n, 1), np.uint8)
        err = np.zeros(max(n, 1), np.float32)
        self._chk(self._lib.orbx_lk_track(self._h, _ptr(prev), w, _ptr(nxt), w, w, h, _ptr(pts), n, _ptr(out), _ptr(st),
                                          _ptr(err), win, max_level, max_iters, epsilon))
        return out[:n].copy(), st[:n].copy(), err[:n].copy()

    def fast_tile_counts(self):
        """(tiles that did the full FAST/NMS work, all tiles) of the last whole-path batch."""
        w, t = C.c_longlong(0), C.c_longlong(0)
        self._chk(self._lib.orbx_fast_tile_counts(self._h, C.byref(w), C.byref(t)))
        return w.value, t.value

    def pyramid_pixel_counts(self):
        """(pyramid pixels produced, all pyramid pixels) of the last whole-path batch (top-rows-first pipeline)."""
        w, t = C.c_longlong(0), C.c_longlong(0)
        self._chk(self._lib.orbx_pyramid_pixel_counts(self._h, C.byref(w), C.byref(t)))
        return w.value, t.value

    def last_stage_times(self, back=0):
        """Stage times (ms) of the timed batched call `back` calls ago; call wait() first."""
        ms = np.zeros(NUM_STAGE_TIMES, np.float32)
        self._chk(self._lib.orbx_stage_times_history(self._h, back, _ptr(ms)))
        return dict(zip(STAGE_NAMES, ms.tolist()))

    def bench_stage(self, n_frames, stage, reps):
        ms = C.c_float(0)
        self._chk(self._lib.orbx_bench_stage(self._h, n_frames, stage, reps, C.byref(ms)))
        return ms.value

    # ---- stage operators (names follow the reference's free functions)
    def fast_score(self, image, threshold, n=9):
        image = _img(image)
        h, w = image.shape
        out = np.zeros((h, w), np.float32)
        self._chk(self._lib.orbx_fast_score(self._h, _ptr(image), w, h, image.strides[0], threshold, n, _ptr(out)))
        return out

    def nms(self, scores, nms_window, nfeatures, threshold=0.0):
        scores = np.ascontiguousarray(scores, dtype=np.float32)
        h, w = scores.shape
        kps = np.zeros((max(nfeatures, 1), 2), np.int32)
        cnt, tot = C.c_int(0), C.c_int(0)
        self._chk(self._lib.orbx_nms(self._h, _ptr(scores), w, h, nms_window, nfeatures, threshold, _ptr(kps),
                                     C.byref(cnt), C.byref(tot)))
        return kps[:cnt.value].copy(), tot.value

    def fast(self, image, threshold, n, nms_window, nfeatures):
        image = _img(image)
        h, w = image.shape
        kps = np.zeros((max(nfeatures, 1), 2), np.int32)
        cnt, tot = C.c_int(0), C.c_int(0)
        self._chk(self._lib.orbx_fast(self._h, _ptr(image), w, h, image.strides[0], threshold, n, nms_window,
                                      nfeatures, _ptr(kps), C.byref(cnt), C.byref(tot)))
        return kps[:cnt.value].copy(), tot.value

    def orientations(self, image, kps, patch_size):
        image = _img(image)
        h, w = image.shape
        kps = _kps(kps)
        out = np.zeros(len(kps), np.float32)
        self._chk(self._lib.orbx_orientations(self._h, _ptr(image), w, h, image.strides[0], _ptr(kps), len(kps),
                                              patch_size, _ptr(out)))
        return out

    def brief(self, image, kps, angles):
        image = _img(image)
        h, w = image.shape
        kps = _kps(kps)
        angles = np.ascontiguousarray(angles, dtype=np.float32)
        out = np.zeros((len(kps), 32), np.uint8)
        self._chk(self._lib.orbx_brief(self._h, _ptr(image), w, h, image.strides[0], _ptr(kps), _ptr(angles), len(kps),
                                       _ptr(out)))
        return out

    def harris(self, image, kps, window=7, k=0.04):
        image = _img(image)
        h, w = image.shape
        kps = _kps(kps)
        out = np.zeros(len(kps), np.float32)
        self._chk(self._lib.orbx_harris(self._h, _ptr(image), w, h, image.strides[0], _ptr(kps), len(kps), window, k,
                                        _ptr(out)))
        return out

    def blur5_sep(self, image):
        image = _img(image)
        h, w = image.shape
        out = np.zeros((h, w), np.uint8)
        self._chk(self._lib.orbx_blur5_sep(self._h, _ptr(image), w, h, image.strides[0], _ptr(out), w))
        return out

    def blur5_273(self, image):
        image = _img(image)
        h, w = image.shape
        out = np.zeros((h, w), np.uint8)
        self._chk(self._lib.orbx_blur5_273(self._h, _ptr(image), w, h, image.strides[0], _ptr(out), w))
        return out

    def conv2d(self, padded, kernel):
        padded = _img(padded)
        h, w = padded.shape
        kernel = np.ascontiguousarray(kernel, dtype=np.float32)
        K = kernel.shape[0]
        out = np.zeros((h - K + 1, w - K + 1), np.uint8)
        self._chk(self._lib.orbx_conv2d(self._h, _ptr(padded), w, h, padded.strides[0], _ptr(kernel), K, _ptr(out)))
        return out

    def gaussian_blur_conv(self, image, K):
        image = _img(image)
        h, w = image.shape
        out = np.zeros((h, w), np.uint8)
        self._chk(self._lib.orbx_gaussian_blur_conv(self._h, _ptr(image), w, h, image.strides[0], K, _ptr(out)))
        return out

    def sobel(self, image, direction):
        image = _img(image)
        h, w = image.shape
        out = np.zeros((h, w), np.uint8)
        self._chk(self._lib.orbx_sobel(self._h, _ptr(image), w, h, image.strides[0], direction, _ptr(out)))
        return out

    def build_pyramid_level(self, image, level):
        image = _img(image)
        h, w = image.shape
        pl = self.plan(w, h)
        out = np.zeros((int(pl["level_h"][level]), int(pl["level_w"][level])), np.uint8)
        lw, lh = C.c_int(0), C.c_int(0)
        self._chk(self._lib.orbx_build_pyramid_level(self._h, _ptr(image), w, h, image.strides[0], level, _ptr(out),
                                                     C.byref(lw), C.byref(lh)))
        assert (lh.value, lw.value) == out.shape
        return out

    def select_top(self, responses, keep):
        responses = np.ascontiguousarray(responses, dtype=np.float32)
        idx = np.zeros(max(len(responses), 1), np.int32)
        kept = C.c_int(0)
        self._chk(self._lib.orbx_select_top(self._h, _ptr(responses), len(responses), keep, _ptr(idx), C.byref(kept)))
        return idx[:kept.value].copy()


class _Matcher:
    def knn2(self, query, train):
        """flann->knnMatch(des1, des2, matches, 2) as exact Hamming 2-NN: (idx[nq,2], dist[nq,2])."""
        q, t = _desc(query), _desc(train)
        idx = np.full((max(len(q), 1), 2), -1, np.int32)
        dist = np.full((max(len(q), 1), 2), -1, np.int32)
        self._chk(self._lib.orbx_knn2(self._h, _ptr(q), len(q), _ptr(t), len(t), _ptr(idx), _ptr(dist)))
        return idx[:len(q)].copy(), dist[:len(q)].copy()

    def match_ratio(self, query, train, ratio=0.8):
        """knnMatch + `m.distance < ratio * n.distance` (feature_matching.cpp:166-181)."""
        q, t = _desc(query), _desc(train)
        n = max(len(q), 1)
        qi, ti, d1 = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        cnt = C.c_int(0)
        self._chk(self._lib.orbx_match_ratio(self._h, _ptr(q), len(q), _ptr(t), len(t), ratio, _ptr(qi), _ptr(ti),
                                             _ptr(d1), n, C.byref(cnt)))
        m = cnt.value
        return qi[:m].copy(), ti[:m].copy(), d1[:m].copy()

    def batch_match_consecutive(self, ratio=0.8):
        self._chk(self._lib.orbx_batch_match_consecutive(self._h, ratio))

    def batch_match_fetch(self, pair, capacity):
        qi, ti, d1 = np.zeros(capacity, np.int32), np.zeros(capacity, np.int32), np.zeros(capacity, np.int32)
        cnt = C.c_int(0)
        self._chk(self._lib.orbx_batch_match_fetch(self._h, pair, _ptr(qi), _ptr(ti), _ptr(d1), capacity,
                                                   C.byref(cnt)))
        m = cnt.value
        return qi[:m].copy(), ti[:m].copy(), d1[:m].copy()


class _Pose:
    """Relative pose: findEssentialMat(RANSAC) + recoverPose (include/orbx.h)."""

    def estimate_pose(self, pts1, pts2, K, prob=0.999, threshold=1.0, max_iters=1000, seed=0):
        """get_pose on (n, 2) point arrays: dict with E, R (3x3), t (3,), mask (n,), inliers, good, iters."""
        p1, p2, n = _point_pairs(pts1, pts2)
        K = _f64(K, (3, 3))
        E, R, t = np.zeros(9), np.zeros(9), np.zeros(3)
        mask = np.zeros(max(n, 1), np.uint8)
        inl, good, iters = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._chk(self._lib.orbx_estimate_pose(self._h, _ptr(p1), _ptr(p2), n, _dp(K), prob, threshold, max_iters,
                                               seed, _ptr(E), _ptr(R), _ptr(t), _ptr(mask), C.byref(inl),
                                               C.byref(good), C.byref(iters)))
        return {"E": E.reshape(3, 3), "R": R.reshape(3, 3), "t": t, "mask": mask[:n], "inliers": inl.value,
                "good": good.value, "iters": iters.value}

    def batch_pose_consecutive(self, K, prob=0.999, threshold=1.0, max_iters=1000, seed=0):
        """Poses every pair of the last batch_match_consecutive on the device (no host round trip)."""
        K = _f64(K, (3, 3))
        self._chk(self._lib.orbx_batch_pose_consecutive(self._h, _dp(K), prob, threshold, max_iters, seed))
        self._pose_pairs = self.batch_view().n - 1

    def batch_pose_fetch(self, first=0, n=None):
        """dict of arrays for pairs [first, first + n): E, R (n, 3, 3), t (n, 3), inliers, good, iters (n,)."""
        n = _count(n, first, getattr(self, "_pose_pairs", 0))
        m = max(n, 0)  # a negative n (nothing posed yet) is the C entry's to refuse
        E, R, t = np.zeros((m, 3, 3)), np.zeros((m, 3, 3)), np.zeros((m, 3))
        inl, good, iters = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.int32)
        self._chk(self._lib.orbx_batch_pose_fetch(self._h, first, n, _ptr(E), _ptr(R), _ptr(t), _ptr(inl), _ptr(good),
                                                  _ptr(iters)))
        return {"E": E, "R": R, "t": t, "inliers": inl, "good": good, "iters": iters}

    def batch_pose_mask(self, pair):
        """final mask of one pair, in batch_match_fetch order."""
        cnt = C.c_int(0)
        st = self._lib.orbx_batch_pose_mask(self._h, pair, None, 0, C.byref(cnt))
        if st not in (OK, ERR_CAPACITY):
            self._chk(st)
        mask = np.zeros(max(cnt.value, 1), np.uint8)
        self._chk(self._lib.orbx_batch_pose_mask(self._h, pair, _ptr(mask), cnt.value, C.byref(cnt)))
        return mask[:cnt.value]


def _valid(v, n):
    if v is None:
        return None
    v = np.ascontiguousarray(np.asarray(v).reshape(-1) != 0, np.uint8)
    if len(v) != n:
        raise ValueError("a valid array and its point list differ in length")
    return v


class _Scale:
    """Triangulation and relative scale: the reference's get_scale (include/orbx.h)."""

    def triangulate(self, pts1, pts2, K, R, t):
        """cv::triangulatePoints(K [I|0], K [R|t], pts1, pts2) + X/w: (xyz (n, 3) float32, valid (n,) uint8)."""
        p1, p2, n = _point_pairs(pts1, pts2)
        K, R, t = _f64(K, (3, 3)), _f64(R, (3, 3)), _f64(t, (3,))
        xyz = np.zeros((max(n, 1), 3), np.float32)
        valid = np.zeros(max(n, 1), np.uint8)
        self._chk(self._lib.orbx_triangulate(self._h, _ptr(p1), _ptr(p2), n, _dp(K), _dp(R), _dp(t), _ptr(xyz),
                                             _ptr(valid)))
        return xyz[:n], valid[:n]

    def estimate_scale(self, prev_xyz, cur_xyz, prev_valid=None, cur_valid=None):
        """The tail of get_scale on two index-aligned point lists: (scale, ratios_used)."""
        a = np.ascontiguousarray(np.asarray(prev_xyz, np.float32).reshape(-1, 3))
        b = np.ascontiguousarray(np.asarray(cur_xyz, np.float32).reshape(-1, 3))
        va, vb = _valid(prev_valid, len(a)), _valid(cur_valid, len(b))
        scale, used = C.c_double(0), C.c_int32(0)
        self._chk(self._lib.orbx_estimate_scale(self._h, _ptr(a), _ptr(va), len(a), _ptr(b), _ptr(vb), len(b),
                                                C.byref(scale), C.byref(used)))
        return scale.value, used.value

    def batch_scale_consecutive(self, K):
        """Triangulates and scales every pair of the last batch_pose_consecutive on the device."""
        self._chk(self._lib.orbx_batch_scale_consecutive(self._h, _dp(_f64(K, (3, 3)))))
        self._scale_pairs = getattr(self, "_pose_pairs", 0)

    def batch_scale_fetch(self, first=0, n=None):
        """dict of arrays for pairs [first, first + n): scale (float64), triplets, ratios_used (int32)."""
        n = _count(n, first, getattr(self, "_scale_pairs", 0))
        m = max(n, 0)  # a negative n (nothing scaled yet) is the C entry's to refuse
        scale, trip, used = np.zeros(m), np.zeros(m, np.int32), np.zeros(m, np.int32)
        self._chk(self._lib.orbx_batch_scale_fetch(self._h, first, n, _ptr(scale), _ptr(trip), _ptr(used)))
        return {"scale": scale, "triplets": trip, "ratios_used": used}

    def batch_points_fetch(self, pair, capacity=None):
        """The triangulated points of one pair in batch_match_fetch order: (xyz (n, 3) float32, valid (n,) uint8).
        capacity=None: sized from the pair's match count."""
        f = self._lib.orbx_batch_points_fetch
        cnt = C.c_int(0)
        if capacity is None:
            st = f(self._h, pair, None, None, 0, C.byref(cnt))
            if st not in (OK, ERR_CAPACITY):
                self._chk(st)
            capacity = cnt.value
        xyz = np.zeros((max(capacity, 1), 3), np.float32)
        valid = np.zeros(max(capacity, 1), np.uint8)
        self._chk(f(self._h, pair, _ptr(xyz), _ptr(valid), capacity, C.byref(cnt)))
        return xyz[:cnt.value], valid[:cnt.value]


class _BundleAdjust:
    """Sliding-window bundle adjustment: the reference's Ceres solve (include/orbx.h)."""

    def bundle_adjust(self, K, poses, points, obs_point, obs_pose, obs_xy, huber_delta=1.0, max_iters=200):
        """One window: (poses (W, 6), points (N, 3), summary dict).  poses: angle-axis + translation, world ->
        camera; pose 0 is constant.  The outputs equal the inputs unless the summary says convergence."""
        K, poses, points = _f64(K, (3, 3)), _f64(poses, (-1, 6), copy=True), _f64(points, (-1, 3), copy=True)
        op, oq, xy = _observations(obs_point, obs_pose, obs_xy)
        out = BaSummary()
        self._chk(self._lib.orbx_bundle_adjust(self._h, _dp(K), len(poses), _dp(poses), len(points), _dp(points),
                                               len(op), _ip(op), _ip(oq), _dp(xy), huber_delta, max_iters,
                                               C.byref(out)))
        return poses, points, out.as_dict()

    def bundle_adjust_batch(self, K, windows, huber_delta=1.0, max_iters=200):
        """Many independent windows in one launch.  windows: a sequence of (poses, points, obs_point, obs_pose,
        obs_xy) with window-local indices; returns a list of (poses, points, summary dict)."""
        n = len(windows)
        cat = lambda k, dt, sh: np.concatenate([np.asarray(w[k], dt).reshape(sh) for w in windows]) if n else np.zeros(sh, dt)
        off = lambda k, sh: _i32(np.concatenate([[0], np.cumsum([len(np.asarray(w[k]).reshape(sh)) for w in windows])]))
        K = _f64(K, (3, 3))
        poses, points = _f64(cat(0, np.float64, (-1, 6)), (-1, 6), copy=True), _f64(cat(1, np.float64, (-1, 3)), (-1, 3), copy=True)
        op, oq, xy = _observations(cat(2, np.int32, (-1,)), cat(3, np.int32, (-1,)), cat(4, np.float64, (-1, 2)))
        po, xo, oo = off(0, (-1, 6)), off(1, (-1, 3)), off(2, (-1,))
        out = (BaSummary * max(n, 1))()
        self._chk(self._lib.orbx_bundle_adjust_batch(self._h, _dp(K), n, _ip(po), _dp(poses), _ip(xo), _dp(points),
                                                     _ip(oo), _ip(op), _ip(oq), _dp(xy), huber_delta, max_iters,
                                                     out))
        return [(poses[po[w]:po[w + 1]], points[xo[w]:xo[w + 1]], out[w].as_dict()) for w in range(n)]


class _GoodFeatures:
    """Shi-Tomasi corners: cv::goodFeaturesToTrack (include/orbx.h)."""

    def corner_min_eigen_val(self, image):
        """cv::cornerMinEigenVal(image, eig, 3, 3): the (h, w) float32 response map."""
        image = _gftt_view(image)
        h, w = image.shape
        out = np.zeros((h, w), np.float32)
        self._chk(self._lib.orbx_corner_min_eigen_val(self._h, _ptr(image), w, h, image.strides[0], _ptr(out)))
        return out

    def good_features_to_track(self, image, max_corners=2000, quality_level=0.01, min_distance=8.0, capacity=None):
        """cv::goodFeaturesToTrack(image, corners, maxCorners, qualityLevel, minDistance) as called at
        with_bundle_adjustment.cpp:586-593: (n, 2) float32 corners (x, y), strongest first.  max_corners <= 0: no
        limit.  capacity=None: sized for the call (max_corners, or every interior pixel)."""
        image = _gftt_view(image)
        h, w = image.shape
        if capacity is None:
            capacity = max_corners if max_corners > 0 else max((w - 2) * (h - 2), 1)
        out = np.zeros((max(capacity, 1), 2), np.float32)
        cnt = C.c_int(0)
        self._chk(self._lib.orbx_good_features_to_track(self._h, _ptr(image), w, h, image.strides[0], max_corners,
                                                        quality_level, min_distance, _ptr(out), capacity,
                                                        C.byref(cnt)))
        return out[:cnt.value].copy()

    def good_features_batch(self, frames, max_corners=2000, quality_level=0.01, min_distance=8.0, stream=None):
        """orbx_good_features_batch_device on (n, h, w) uint8 frames: a torch device tensor (any strides with unit
        pixel stride; the caller has synchronised its producer, or passes the producer's stream) or a numpy array
        (copied to the device first).  Asynchronous; good_features_fetch delivers the results."""
        frames, n, h, w, rs, fs, uploaded = _frames_arg(frames)
        _sync_uploads(uploaded)
        self._gf_frames = frames  # kept alive until the next batch
        self._chk(self._lib.orbx_good_features_batch_device(self._h, frames.data_ptr(), n, w, h, rs, fs, max_corners,
                                                            quality_level, min_distance, _stream(stream)))

    def good_features_view(self):
        """The device-side result block of the last good-features batch (orbx_good_features_results_device)."""
        v = GoodFeaturesView()
        self._chk(self._lib.orbx_good_features_results_device(self._h, C.byref(v)))
        return v

    def good_features_fetch(self, first=0, n=None):
        """Results of frames [first, first + n) of the last good-features batch: a list of (count, 2) float32 arrays."""
        v = self.good_features_view()
        n = _count(n, first, v.n)
        counts = np.zeros(max(n, 1), np.int32)
        xy = np.zeros((max(n, 1), v.slot_capacity, 2), np.float32)
        self._chk(self._lib.orbx_good_features_fetch(self._h, first, n, _ptr(counts), _ptr(xy)))
        return [xy[i, :counts[i]].copy() for i in range(n)]

    def good_features_workspace_limit(self, nbytes):
        """Bound of the good-features workspace in bytes (0: the default); a larger batch runs in slices."""
        self._chk(self._lib.orbx_good_features_workspace_limit(self._h, nbytes))


class _GoodFeaturesTopup:
    """Masked Shi-Tomasi detection that tops up tracked points (include/orbx.h)."""

    def good_features_topup(self, frames, seeds, seen=None, seen_min=0, seed_capacity=None, seed_point_stride=2,
                            seed_frame_stride=None, max_corners=2000, quality_level=0.01, min_distance=8.0,
                            stream=None):
        """orbx_good_features_topup_device.  frames: (n, h, w) uint8, a torch device tensor (any strides with unit
        pixel stride) or a numpy array (copied to the device first).  seeds: (n, seed_capacity, 2) float32 as a torch
        device tensor or a numpy array, or a raw device address with seed_capacity, seed_point_stride and
        seed_frame_stride (in floats) -- e.g. tracks_xy + 8 * (window_len - 1) of lk_windows_view().  seen:
        (n, seed_capacity) int32 likewise, or None.  Device tensors: the caller has synchronised their producer, or
        passes the producer's stream.  Asynchronous; good_features_topup_fetch delivers the results."""
        frames, n, h, w, rs, fs, up_frames = _frames_arg(frames)
        keep = [frames]
        seeds, t, up_seeds = _device_arg(seeds, np.float32,
                                         lambda t: t.dim() == 3 and t.shape[0] == n and t.shape[2] == 2,
                                         "seeds must be (n, seed_capacity, 2) float32, contiguous, on the device", keep)
        if t is not None:
            seed_capacity, seed_point_stride, seed_frame_stride = t.shape[1], 2, 2 * t.shape[1]
        elif seed_capacity is None or seed_frame_stride is None:
            raise ValueError("a raw seed address needs seed_capacity and seed_frame_stride")
        seen, _, up_seen = _device_arg(seen, np.int32, lambda t: t.numel() == n * seed_capacity,
                                       "seen must be (n, seed_capacity) int32, contiguous, on the device", keep)
        _sync_uploads(up_frames, up_seeds, up_seen)
        self._gft_keep = keep  # kept alive until the next call
        self._chk(self._lib.orbx_good_features_topup_device(
            self._h, frames.data_ptr(), n, w, h, rs, fs, seeds, seed_point_stride, seed_frame_stride, seen, seen_min,
            seed_capacity, max_corners, quality_level, min_distance, _stream(stream)))

    def good_features_topup_view(self):
        """The device-side result block of the last top-up (orbx_good_features_topup_results_device)."""
        v = GoodFeaturesTopupView()
        self._chk(self._lib.orbx_good_features_topup_results_device(self._h, C.byref(v)))
        return v

    def good_features_topup_fetch(self, first=0, n=None):
        """Frames [first, first + n) of the last top-up as whole arrays: counts (n,), carried (n,), points
        (n, slot_capacity, 2) float32 and origin (n, slot_capacity) int32 -- zero / -1 at and beyond counts[f]."""
        v = self.good_features_topup_view()
        n = _count(n, first, v.n)
        m = max(n, 1)
        counts, carried = np.zeros(m, np.int32), np.zeros(m, np.int32)
        points = np.zeros((m, v.slot_capacity, 2), np.float32)
        origin = np.zeros((m, v.slot_capacity), np.int32)
        self._chk(self._lib.orbx_good_features_topup_fetch(self._h, first, n, _ptr(counts), _ptr(carried),
                                                           _ptr(points), _ptr(origin)))
        return counts, carried, points, origin

    def good_features_topup_one(self, image, seeds, max_corners=2000, quality_level=0.01, min_distance=8.0,
                                capacity=None):
        """orbx_good_features_topup on one host image and (n, 2) host seeds: points (count, 2) float32, origin
        (count,) int32 and the number of carried points."""
        image = _gftt_view(image)
        h, w = image.shape
        seeds = np.ascontiguousarray(seeds, np.float32).reshape(-1, 2)
        if capacity is None:
            capacity = max(max_corners, 1)
        points = np.zeros((max(capacity, 1), 2), np.float32)
        origin = np.zeros(max(capacity, 1), np.int32)
        cnt, car = C.c_int(0), C.c_int(0)
        self._chk(self._lib.orbx_good_features_topup(
            self._h, _ptr(image), w, h, image.strides[0], _ptr(seeds) if len(seeds) else None, len(seeds), max_corners,
            quality_level, min_distance, _ptr(points), _ptr(origin), capacity, C.byref(cnt), C.byref(car)))
        return points[:cnt.value].copy(), origin[:cnt.value].copy(), car.value

    def good_features_to_track_masked(self, image, mask, max_corners=2000, quality_level=0.01, min_distance=8.0,
                                      capacity=None):
        """cv::goodFeaturesToTrack(image, corners, maxCorners, qualityLevel, minDistance, mask): (n, 2) float32
        corners; a pixel whose mask byte is 0 is no corner.  max_corners <= 0: no limit."""
        image = _gftt_view(image)
        h, w = image.shape
        mask = _gftt_view(mask)
        if mask.shape != image.shape:
            raise ValueError("mask and image differ in size")
        if capacity is None:
            capacity = max_corners if max_corners > 0 else max((w - 2) * (h - 2), 1)
        out = np.zeros((max(capacity, 1), 2), np.float32)
        cnt = C.c_int(0)
        self._chk(self._lib.orbx_good_features_to_track_masked(
            self._h, _ptr(image), w, h, image.strides[0], _ptr(mask), mask.strides[0], max_corners, quality_level,
            min_distance, _ptr(out), capacity, C.byref(cnt)))
        return out[:cnt.value].copy()


class _LkWindows:
    """Lucas-Kanade over frame windows: trackPointsAcrossWindow for many windows per launch (include/orbx.h;
    DESIGN.md §9 rank 9), with the forward-backward check when fb_threshold is given (rank 13)."""

    def lk_track_windows(self, frames, window_first, window_len, points, counts=None, win=21, max_level=3,
                         max_iters=30, epsilon=0.01, slot_capacity=None, stream=None, fb_threshold=None):
        """orbx_lk_track_windows_device, or orbx_lk_track_windows_fb_device when fb_threshold is not None (then
        lk_windows_fb_fetch delivers fb_d2 and lost beside the usual results).  frames: (n, h, w) uint8, a torch device tensor (any strides with unit pixel
        stride; read in place) or a numpy array (copied to the device first).  points: (n_windows, slot_capacity, 2)
        float32 and counts: (n_windows,) int32 or None, each a torch device tensor, a numpy array or a raw device
        address (then slot_capacity is required) -- e.g. the fields of good_features_view().  Device tensors: the
        caller has synchronised their producer, or passes the producer's stream.  Asynchronous; lk_windows_fetch
        delivers the results."""
        frames, n, h, w, rs, fs, up_frames = _frames_arg(frames)
        window_first = np.ascontiguousarray(window_first, np.int32).reshape(-1)
        nw = len(window_first)
        keep = [frames]
        points, slot_capacity, up_points = _lk_points_arg(points, nw, slot_capacity, keep)
        counts, _, up_counts = _device_arg(counts, np.int32, lambda t: t.numel() == nw,
                                           "counts must be (n_windows,) int32, contiguous, on the device", keep)
        _sync_uploads(up_frames, up_points, up_counts)
        self._lkw_keep = keep  # kept alive until the next call
        args = [self._h, frames.data_ptr(), n, w, h, rs, fs, _ptr(window_first), nw, window_len, points, counts,
                slot_capacity, win, max_level, max_iters, epsilon]
        if fb_threshold is None:
            self._chk(self._lib.orbx_lk_track_windows_device(*args, _stream(stream)))
        else:
            self._chk(self._lib.orbx_lk_track_windows_fb_device(*args, fb_threshold, _stream(stream)))

    def lk_windows_view(self):
        """The device-side result block of the last windows call (orbx_lk_windows_results_device)."""
        v = LkWindowsView()
        self._chk(self._lib.orbx_lk_windows_results_device(self._h, C.byref(v)))
        return v

    def lk_windows_fetch(self, first=0, n=None):
        """Windows [first, first + n) of the last windows call: tracks (n, slots, window_len, 2) float32, seen
        (n, slots) int32, err (n, slots, window_len - 1) float32, zero past `seen` and in unused slots."""
        v = self.lk_windows_view()
        n = _count(n, first, v.n_windows)
        m = max(n, 1)
        tracks = np.zeros((m, v.slot_capacity, v.window_len, 2), np.float32)
        seen = np.zeros((m, v.slot_capacity), np.int32)
        err = np.zeros((m, v.slot_capacity, v.window_len - 1), np.float32)
        self._chk(self._lib.orbx_lk_windows_fetch(self._h, first, n, _ptr(tracks), _ptr(seen), _ptr(err)))
        return tracks, seen, err

    def lk_windows_fb_view(self):
        """What the forward-backward check added to the last windows call, on the device
        (orbx_lk_windows_fb_results_device); raises after a call without the check."""
        v = LkWindowsFbView()
        self._chk(self._lib.orbx_lk_windows_fb_results_device(self._h, C.byref(v)))
        return v

    def lk_windows_fb_fetch(self, first=0, n=None):
        """Windows [first, first + n) of the last windows call with the check: fb_d2 (n, slots, window_len - 1)
        float32, the squared forward-backward distance of every pair that passed, and lost (n, slots) int32, 0 or the
        reason the track ended (LK_FB_FORWARD / LK_FB_BACKWARD / LK_FB_DISTANCE)."""
        v = self.lk_windows_fb_view()
        n = _count(n, first, v.n_windows)
        m = max(n, 1)
        fb_d2 = np.zeros((m, v.slot_capacity, v.window_len - 1), np.float32)
        lost = np.zeros((m, v.slot_capacity), np.int32)
        self._chk(self._lib.orbx_lk_windows_fb_fetch(self._h, first, n, _ptr(fb_d2), _ptr(lost)))
        return fb_d2, lost

    def lk_workspace_limit(self, nbytes):
        """Bound of the windows workspace in bytes (0: the default); more frames run in slices of whole windows."""
        self._chk(self._lib.orbx_lk_workspace_limit(self._h, nbytes))

    def lk_track_window(self, frames, pts, win=21, max_level=3, max_iters=30, epsilon=0.01, fb_threshold=None):
        """orbx_lk_track_window: one window of host frames (n_frames, h, w) and host points (n, 2).  Returns tracks
        (n, n_frames, 2), seen (n,), err (n, n_frames - 1); with fb_threshold (orbx_lk_track_window_fb) also fb_d2
        (n, n_frames - 1) and lost (n,)."""
        frames = np.ascontiguousarray(frames, np.uint8)
        if frames.ndim != 3:
            raise ValueError("frames must be (n_frames, h, w) uint8")
        nf, h, w = frames.shape
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        n = len(pts)
        tracks = np.zeros((max(n, 1), nf, 2), np.float32)
        seen = np.zeros(max(n, 1), np.int32)
        err = np.zeros((max(n, 1), max(nf - 1, 1)), np.float32)
        args = [self._h, _ptr(frames), nf, w, h, w, w * h, _ptr(pts), n, _ptr(tracks), _ptr(seen), _ptr(err), win,
                max_level, max_iters, epsilon]
        if fb_threshold is None:
            self._chk(self._lib.orbx_lk_track_window(*args))
            return tracks[:n].copy(), seen[:n].copy(), err[:n, :nf - 1].copy()
        fb_d2 = np.zeros_like(err)
        lost = np.zeros(max(n, 1), np.int32)
        self._chk(self._lib.orbx_lk_track_window_fb(*args, fb_threshold, _ptr(fb_d2), _ptr(lost)))
        return tracks[:n].copy(), seen[:n].copy(), err[:n, :nf - 1].copy(), fb_d2[:n, :nf - 1].copy(), lost[:n].copy()


class _Landmarks:
    """Landmarks of tracked windows built on the device and bundle-adjusted there:
    buildLandmarksFromFirstTwoFramesAndTracks + the window's solve (include/orbx.h)."""

    def landmarks_build(self, K, tracks, seen, poses, n_windows=None, slot_capacity=None, window_len=None,
                        stream=None):
        """orbx_landmarks_build_device.  tracks: (n_windows, slots, window_len, 2) float32 and seen: (n_windows,
        slots) int32, each a torch device tensor, a numpy array (copied to the device first) or a raw device address
        (then n_windows, slot_capacity and window_len are required) -- e.g. the fields of lk_windows_view().  poses:
        host, (n_windows, window_len, 6).  Asynchronous; landmarks_fetch delivers the block."""
        tracks, seen, n_windows, slot_capacity, window_len, self._lm_keep = _tracks_args(
            tracks, seen, n_windows, slot_capacity, window_len)  # (the tensors: kept alive until the next build)
        K, poses = _f64(K, (3, 3)), _f64(poses, (-1, 6))
        if len(poses) != max(n_windows, 0) * max(window_len, 0):
            raise ValueError("poses must be (n_windows, window_len, 6)")
        self._chk(self._lib.orbx_landmarks_build_device(self._h, _dp(K), tracks, seen, n_windows, slot_capacity,
                                                        window_len, _dp(poses), _stream(stream)))

    def landmarks_view(self):
        """The device-side landmarks block of the last build (orbx_landmarks_results_device)."""
        v = LandmarksView()
        self._chk(self._lib.orbx_landmarks_results_device(self._h, C.byref(v)))
        return v

    def landmarks_fetch(self, first=0, n=None):
        """Windows [first, first + n) of the last build in the format of bundle_adjust_batch: a dict of status (n),
        pose_offset / point_offset / obs_offset (n + 1), points3 (N, 3), slot_of_point (N), obs_point / obs_pose (M)
        and obs_xy (M, 2)."""
        n = _count(n, first, lambda: self.landmarks_view().n_windows)
        f = self._lib.orbx_landmarks_fetch
        npt, nob = C.c_int(0), C.c_int(0)
        self._chk(f(self._h, first, n, None, None, None, None, None, None, 0, None, None, None, 0, C.byref(npt),
                    C.byref(nob)))
        N, M, m = npt.value, nob.value, max(n, 1)
        out = dict(status=np.zeros(m, np.int32), pose_offset=np.zeros(m + 1, np.int32),
                   point_offset=np.zeros(m + 1, np.int32), obs_offset=np.zeros(m + 1, np.int32),
                   points3=np.zeros((N, 3)), slot_of_point=np.zeros(N, np.int32), obs_point=np.zeros(M, np.int32),
                   obs_pose=np.zeros(M, np.int32), obs_xy=np.zeros((M, 2)))
        p = lambda k: _ptr(out[k]) if out[k].size else None
        self._chk(f(self._h, first, n, p("status"), p("pose_offset"), p("point_offset"), p("obs_offset"),
                    p("points3"), p("slot_of_point"), N, p("obs_point"), p("obs_pose"), p("obs_xy"), M,
                    C.byref(npt), C.byref(nob)))
        return out

    def bundle_adjust_landmarks(self, huber_delta=1.0, max_iters=200, stream=None):
        """orbx_bundle_adjust_landmarks_device: solves every window of the last landmarks block.  Asynchronous;
        bundle_adjust_landmarks_fetch delivers the results."""
        self._chk(self._lib.orbx_bundle_adjust_landmarks_device(self._h, huber_delta, max_iters, _stream(stream)))

    def bundle_adjust_landmarks_fetch(self, first=0, n=None, points=True):
        """Windows [first, first + n) of the last solve: poses (n, window_len, 6), a list of summary dicts, and the
        points (N, 3) in the order of the block (None with points=False)."""
        v = self.landmarks_view()
        n = _count(n, first, v.n_windows)
        m = max(n, 1)
        poses = np.zeros((m, v.window_len, 6))
        out = (BaSummary * m)()
        f = self._lib.orbx_bundle_adjust_landmarks_fetch
        cnt = C.c_int(0)
        pts = None
        if points:
            self._chk(f(self._h, first, n, None, None, None, 0, C.byref(cnt)))
            pts = np.zeros((cnt.value, 3))
        self._chk(f(self._h, first, n, _ptr(poses), out, _ptr(pts) if points and pts.size else None, cnt.value,
                    C.byref(cnt)))
        return poses[:n], [out[w].as_dict() for w in range(n)], pts

    def bundle_adjust_tracks(self, K, tracks, seen, poses, huber_delta=1.0, max_iters=200):
        """orbx_bundle_adjust_tracks: one window of host tracks (slots, window_len, 2), seen (slots) and poses
        (window_len, 6) through both stages.  Returns (poses, summary dict, landmarks status, points (N, 3),
        slot_of_point (N))."""
        tracks, seen, slots, wl = _host_window(tracks, seen)
        K, poses = _f64(K, (3, 3)), _f64(poses, (-1, 6), copy=True)
        if len(poses) != wl:
            raise ValueError("poses must be (window_len, 6)")
        pts = np.zeros((max(slots, 1), 3))
        sop = np.zeros(max(slots, 1), np.int32)
        st, cnt, out = C.c_int32(-1), C.c_int(0), BaSummary()
        self._chk(self._lib.orbx_bundle_adjust_tracks(self._h, _dp(K), _ptr(tracks), _ptr(seen), slots, wl,
                                                      _dp(poses), huber_delta, max_iters, C.byref(st), C.byref(out),
                                                      _ptr(pts), _ptr(sop), slots, C.byref(cnt)))
        return poses, out.as_dict(), st.value, pts[:cnt.value].copy(), sop[:cnt.value].copy()


_TRACKS_POSE_ORDER = ("E", "R", "t", "inliers", "good", "iters", "n", "scale", "triplets", "ratios_used")


def _tracks_pose_arrays(m):
    return dict(E=np.zeros((m, 3, 3)), R=np.zeros((m, 3, 3)), t=np.zeros((m, 3)), inliers=np.zeros(m, np.int32),
                good=np.zeros(m, np.int32), iters=np.zeros(m, np.int32), n=np.zeros(m, np.int32),
                scale=np.zeros(m), triplets=np.zeros(m, np.int32), ratios_used=np.zeros(m, np.int32))


class _TracksPose:
    """Pose, triangulated points and relative scale of every consecutive frame pair of tracked windows, from the
    tracks block on the device (include/orbx.h)."""

    def tracks_pose(self, K, tracks, seen=None, n_windows=None, slot_capacity=None, window_len=None, prob=0.999,
                    threshold=1.0, max_iters=1000, seed=0, stream=None):
        """orbx_tracks_pose_device.  tracks: an LkWindowsView (lk_windows_view(); seen and the three sizes come from
        it), or (n_windows, slots, window_len, 2) float32 with seen (n_windows, slots) int32, each a torch device
        tensor, a numpy array (copied to the device first) or a raw device address (then n_windows, slot_capacity and
        window_len are required).  Asynchronous; tracks_pose_fetch / tracks_pose_pair_fetch deliver the block."""
        tracks, seen, n_windows, slot_capacity, window_len, self._tp_keep = _tracks_args(
            tracks, seen, n_windows, slot_capacity, window_len)  # (the tensors: kept alive until the next call)
        K = _f64(K, (3, 3))
        self._chk(self._lib.orbx_tracks_pose_device(self._h, _dp(K), tracks, seen, n_windows, slot_capacity,
                                                    window_len, prob, threshold, max_iters, seed, _stream(stream)))

    def tracks_pose_view(self):
        """The device-side block of the last tracks_pose (orbx_tracks_pose_results_device)."""
        v = TracksPoseView()
        self._chk(self._lib.orbx_tracks_pose_results_device(self._h, C.byref(v)))
        return v

    def tracks_pose_fetch(self, first=0, n=None):
        """Pairs [first, first + n) of the last tracks_pose (pair p = w * (window_len - 1) + k): dict of E, R
        (n, 3, 3), t (n, 3), inliers, good, iters, n (the list lengths), scale, triplets, ratios_used."""
        n = _count(n, first, lambda: self.tracks_pose_view().n_pairs)
        out = _tracks_pose_arrays(max(n, 0))
        self._chk(self._lib.orbx_tracks_pose_fetch(self._h, first, n, *[_ptr(out[k]) for k in _TRACKS_POSE_ORDER]))
        return out

    def tracks_pose_pair_fetch(self, pair, capacity=None):
        """The lists of one pair, one entry per surviving slot in ascending slot order: dict of slot_of (n,) int32,
        mask (n,) uint8, xyz (n, 3) float32, valid (n,) uint8.  capacity=None: sized from the pair's count."""
        f = self._lib.orbx_tracks_pose_pair_fetch
        cnt = C.c_int(0)
        if capacity is None:
            st = f(self._h, pair, None, None, None, None, 0, C.byref(cnt))
            if st not in (OK, ERR_CAPACITY):
                self._chk(st)
            capacity = cnt.value
        m = max(capacity, 1)
        slot_of, mask = np.zeros(m, np.int32), np.zeros(m, np.uint8)
        xyz, valid = np.zeros((m, 3), np.float32), np.zeros(m, np.uint8)
        self._chk(f(self._h, pair, _ptr(slot_of), _ptr(mask), _ptr(xyz), _ptr(valid), capacity, C.byref(cnt)))
        k = cnt.value
        return {"slot_of": slot_of[:k], "mask": mask[:k], "xyz": xyz[:k], "valid": valid[:k]}

    def tracks_pose_window(self, K, tracks, seen, prob=0.999, threshold=1.0, max_iters=1000, seed=0):
        """orbx_tracks_pose: one window of host tracks (slots, window_len, 2) and seen (slots).  Returns the dict of
        tracks_pose_fetch for the window's window_len - 1 pairs; tracks_pose_pair_fetch delivers their lists."""
        tracks, seen, slots, wl = _host_window(tracks, seen)
        K = _f64(K, (3, 3))
        out = _tracks_pose_arrays(max(wl - 1, 0))
        self._chk(self._lib.orbx_tracks_pose(self._h, _dp(K), _ptr(tracks), _ptr(seen), slots, wl, prob, threshold,
                                             max_iters, seed, *[_ptr(out[k]) for k in _TRACKS_POSE_ORDER]))
        return out


class Context(_Core, _Matcher, _Pose, _Scale, _BundleAdjust, _GoodFeatures, _GoodFeaturesTopup, _LkWindows,
              _Landmarks, _TracksPose):
    """One orbx_ctx: single-threaded, owns all device memory, one per GPU."""


def chain_trajectory(T0, R, t, scale):
    """cur_pose = cur_pose * T.inv(), T = [R | scale * t], over n relative motions (feature_matching.cpp:77-82):
    (n + 1, 4, 4) poses with poses[0] = T0.  Host only."""
    T0, R, t, scale = _f64(T0, (4, 4)), _f64(R, (-1, 3, 3)), _f64(t, (-1, 3)), _f64(scale, (-1,))
    n = len(R)
    if len(t) != n or len(scale) != n:
        raise ValueError("R, t and scale differ in length")
    poses = np.zeros((n + 1, 4, 4))
    st = load().orbx_chain_trajectory(_dp(T0), _dp(R), _dp(t), _dp(scale), n, _dp(poses))
    if st != OK:
        raise OrbxError(st, "orbx_chain_trajectory")
    return poses


def gaussian_kernel(K, sigma=-1.0):
    out = np.zeros(K * K, np.float32)
    st = load().orbx_gaussian_kernel(K, sigma, _ptr(out))
    if st != OK:
        raise OrbxError(st, "orbx_gaussian_kernel")
    return out.reshape(K, K)


def version():
    return load().orbx_version().decode()
