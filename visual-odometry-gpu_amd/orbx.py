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

# every symbol include/orbx.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "orbx_params_default_gpu", "orbx_params_default_cpu", "orbx_create", "orbx_destroy",
    "orbx_last_error_string", "orbx_status_string", "orbx_version", "orbx_get_plan",
    "orbx_detect_and_compute", "orbx_detect_and_compute_batch_device", "orbx_detect_and_compute_batch_host",
    "orbx_wait", "orbx_batch_results_device", "orbx_batch_results_host", "orbx_batch_fetch", "orbx_batch_prefetch", "orbx_batch_prefetch_compact",
    "orbx_batch_fetch_previous", "orbx_enable_stage_timing",
    "orbx_last_stage_times", "orbx_stage_times_history", "orbx_bench_stage", "orbx_set_fast_early_exit",
    "orbx_set_fused_pyramid_blur", "orbx_set_top_rows_first", "orbx_set_pipelined_batches", "orbx_set_host_results", "orbx_fast_tile_counts", "orbx_pyramid_pixel_counts", "orbx_lk_track", "orbx_lk_pyramid_levels", "orbx_fast_score", "orbx_nms", "orbx_fast",
    "orbx_orientations", "orbx_brief", "orbx_harris", "orbx_blur5_sep", "orbx_blur5_273", "orbx_conv2d",
    "orbx_gaussian_blur_conv", "orbx_gaussian_kernel", "orbx_sobel", "orbx_build_pyramid_level",
    "orbx_select_top", "orbx_knn2", "orbx_match_ratio", "orbx_batch_match_consecutive", "orbx_batch_match_fetch",
    "orbx_estimate_pose", "orbx_batch_pose_consecutive", "orbx_batch_pose_fetch", "orbx_batch_pose_mask",
    "orbx_triangulate", "orbx_estimate_scale", "orbx_batch_scale_consecutive", "orbx_batch_scale_fetch",
    "orbx_batch_points_fetch", "orbx_chain_trajectory", "orbx_debug_fill_pools",
    "orbx_debug_read_pyramid_level",
    "orbx_bundle_adjust", "orbx_bundle_adjust_batch",
    "orbx_corner_min_eigen_val", "orbx_good_features_to_track", "orbx_good_features_batch_device",
    "orbx_good_features_workspace_limit", "orbx_good_features_results_device", "orbx_good_features_fetch",
    "orbx_lk_track_windows_device", "orbx_lk_windows_results_device", "orbx_lk_windows_fetch",
    "orbx_lk_workspace_limit", "orbx_lk_track_window",
    "orbx_landmarks_build_device", "orbx_landmarks_results_device", "orbx_landmarks_fetch",
    "orbx_bundle_adjust_landmarks_device", "orbx_bundle_adjust_landmarks_fetch", "orbx_bundle_adjust_tracks",
    "orbx_tracks_pose_device", "orbx_tracks_pose_results_device", "orbx_tracks_pose_fetch",
    "orbx_tracks_pose_pair_fetch", "orbx_tracks_pose",
    "orbx_good_features_topup_device", "orbx_good_features_topup_results_device", "orbx_good_features_topup_fetch",
    "orbx_good_features_topup", "orbx_good_features_to_track_masked",
    "orbx_lk_track_windows_fb_device", "orbx_lk_windows_fb_results_device", "orbx_lk_windows_fb_fetch",
    "orbx_lk_track_window_fb",
]


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
    """Load liborbx.so (raises OSError if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError("liborbx.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `make -C visual-odometry-gpu_amd/csrc` (there is no CPU fallback)")
        _share_hip_runtime_with_torch()
        lib = C.CDLL(LIB_PATH)
        lib.orbx_last_error_string.restype = C.c_char_p
        lib.orbx_last_error_string.argtypes = [C.c_void_p]
        lib.orbx_status_string.restype = C.c_char_p
        lib.orbx_version.restype = C.c_char_p
        lib.orbx_create.argtypes = [C.POINTER(Params), C.POINTER(C.c_void_p)]
        lib.orbx_destroy.argtypes = [C.c_void_p]
        lib.orbx_destroy.restype = None
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


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _img(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.ndim != 2:
        raise ValueError("image must be 2-D uint8")
    return a


def _kps(k):
    k = np.ascontiguousarray(k, dtype=np.int32).reshape(-1, 2)
    return k


class Context:
    """One orbx_ctx: single-threaded, owns all device memory, one per GPU."""

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
        self._dac.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6 + [
            C.c_int, C.POINTER(C.c_int)]

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
        self._chk(self._lib.orbx_detect_and_compute_batch_device(
            self._h, C.c_void_p(d_ptr), n, width, height, row_stride, C.c_size_t(frame_stride),
            C.c_void_p(stream) if stream else None))

    def batch_host(self, frames):
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if frames.ndim != 3:
            raise ValueError("frames must be (n, h, w) uint8")
        n, h, w = frames.shape
        self._chk(self._lib.orbx_detect_and_compute_batch_host(self._h, _ptr(frames), n, w, h, w, C.c_size_t(w * h)))

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
        self._chk(self._lib.orbx_debug_read_pyramid_level(self._h, int(frame), int(level), _ptr(out), C.c_size_t(out.size)))
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
        f = self._lib.orbx_lk_track
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double]
        self._chk(f(self._h, _ptr(prev), w, _ptr(nxt), w, w, h, _ptr(pts), n, _ptr(out), _ptr(st), _ptr(err), win,
                    max_level, max_iters, epsilon))
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
        self._chk(self._lib.orbx_nms(self._h, _ptr(scores), w, h, nms_window, nfeatures, C.c_float(threshold),
                                     _ptr(kps), C.byref(cnt), C.byref(tot)))
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
        self._chk(self._lib.orbx_harris(self._h, _ptr(image), w, h, image.strides[0], _ptr(kps), len(kps), window,
                                        C.c_float(k), _ptr(out)))
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


def _desc(d):
    d = np.ascontiguousarray(d, dtype=np.uint8).reshape(-1, 32)
    return d


def _matcher_methods():
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
        self._chk(self._lib.orbx_match_ratio(self._h, _ptr(q), len(q), _ptr(t), len(t), C.c_double(ratio), _ptr(qi),
                                             _ptr(ti), _ptr(d1), n, C.byref(cnt)))
        m = cnt.value
        return qi[:m].copy(), ti[:m].copy(), d1[:m].copy()

    def batch_match_consecutive(self, ratio=0.8):
        self._chk(self._lib.orbx_batch_match_consecutive(self._h, C.c_double(ratio)))

    def batch_match_fetch(self, pair, capacity):
        qi, ti, d1 = np.zeros(capacity, np.int32), np.zeros(capacity, np.int32), np.zeros(capacity, np.int32)
        cnt = C.c_int(0)
        self._chk(self._lib.orbx_batch_match_fetch(self._h, pair, _ptr(qi), _ptr(ti), _ptr(d1), capacity,
                                                   C.byref(cnt)))
        m = cnt.value
        return qi[:m].copy(), ti[:m].copy(), d1[:m].copy()

    for f in (knn2, match_ratio, batch_match_consecutive, batch_match_fetch):
        setattr(Context, f.__name__, f)


_matcher_methods()


POSE_MAX_ITERS = 100000  # ORBX_POSE_MAX_ITERS


def _pose_methods():
    """Relative pose: findEssentialMat(RANSAC) + recoverPose (include/orbx.h)."""

    def _K(K):
        K = np.ascontiguousarray(np.asarray(K, np.float64).reshape(3, 3))
        return K, K.ctypes.data_as(C.POINTER(C.c_double))

    def estimate_pose(self, pts1, pts2, K, prob=0.999, threshold=1.0, max_iters=1000, seed=0):
        """get_pose on (n, 2) point arrays: dict with E, R (3x3), t (3,), mask (n,), inliers, good, iters."""
        p1 = np.ascontiguousarray(np.asarray(pts1, np.float32).reshape(-1, 2))
        p2 = np.ascontiguousarray(np.asarray(pts2, np.float32).reshape(-1, 2))
        if p1.shape != p2.shape:
            raise ValueError("pts1 and pts2 differ in shape")
        n = p1.shape[0]
        K, kp = _K(K)
        E, R, t = np.zeros(9), np.zeros(9), np.zeros(3)
        mask = np.zeros(max(n, 1), np.uint8)
        inl, good, iters = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        f = self._lib.orbx_estimate_pose
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_double, C.c_double,
                      C.c_int, C.c_uint64] + [C.c_void_p] * 7
        self._chk(f(self._h, _ptr(p1), _ptr(p2), n, kp, prob, threshold, max_iters, seed, _ptr(E), _ptr(R), _ptr(t),
                    _ptr(mask), C.byref(inl), C.byref(good), C.byref(iters)))
        return {"E": E.reshape(3, 3), "R": R.reshape(3, 3), "t": t, "mask": mask[:n], "inliers": inl.value,
                "good": good.value, "iters": iters.value}

    def batch_pose_consecutive(self, K, prob=0.999, threshold=1.0, max_iters=1000, seed=0):
        """Poses every pair of the last batch_match_consecutive on the device (no host round trip)."""
        K, kp = _K(K)
        f = self._lib.orbx_batch_pose_consecutive
        f.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_double, C.c_double, C.c_int, C.c_uint64]
        self._chk(f(self._h, kp, prob, threshold, max_iters, seed))
        v = BatchView()
        self._chk(self._lib.orbx_batch_results_device(self._h, C.byref(v)))
        self._pose_pairs = v.n - 1

    def batch_pose_fetch(self, first=0, n=None):
        """dict of arrays for pairs [first, first + n): E, R (n, 3, 3), t (n, 3), inliers, good, iters (n,)."""
        if n is None:
            n = getattr(self, "_pose_pairs", 0) - first
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

    for f in (estimate_pose, batch_pose_consecutive, batch_pose_fetch, batch_pose_mask):
        setattr(Context, f.__name__, f)


_pose_methods()


def _scale_methods():
    """Triangulation and relative scale: the reference's get_scale (include/orbx.h)."""
    DP = C.POINTER(C.c_double)

    def _d(a, shape):
        a = np.ascontiguousarray(np.asarray(a, np.float64).reshape(shape))
        return a, a.ctypes.data_as(DP)

    def _valid(v, n):
        if v is None:
            return None
        v = np.ascontiguousarray(np.asarray(v).reshape(-1) != 0, np.uint8)
        if len(v) != n:
            raise ValueError("a valid array and its point list differ in length")
        return v

    def triangulate(self, pts1, pts2, K, R, t):
        """cv::triangulatePoints(K [I|0], K [R|t], pts1, pts2) + X/w: (xyz (n, 3) float32, valid (n,) uint8)."""
        p1 = np.ascontiguousarray(np.asarray(pts1, np.float32).reshape(-1, 2))
        p2 = np.ascontiguousarray(np.asarray(pts2, np.float32).reshape(-1, 2))
        if p1.shape != p2.shape:
            raise ValueError("pts1 and pts2 differ in shape")
        n = p1.shape[0]
        (K, kp), (R, rp), (t, tp) = _d(K, (3, 3)), _d(R, (3, 3)), _d(t, (3,))
        xyz = np.zeros((max(n, 1), 3), np.float32)
        valid = np.zeros(max(n, 1), np.uint8)
        f = self._lib.orbx_triangulate
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, DP, DP, DP, C.c_void_p, C.c_void_p]
        self._chk(f(self._h, _ptr(p1), _ptr(p2), n, kp, rp, tp, _ptr(xyz), _ptr(valid)))
        return xyz[:n], valid[:n]

    def estimate_scale(self, prev_xyz, cur_xyz, prev_valid=None, cur_valid=None):
        """The tail of get_scale on two index-aligned point lists: (scale, ratios_used)."""
        a = np.ascontiguousarray(np.asarray(prev_xyz, np.float32).reshape(-1, 3))
        b = np.ascontiguousarray(np.asarray(cur_xyz, np.float32).reshape(-1, 3))
        va, vb = _valid(prev_valid, len(a)), _valid(cur_valid, len(b))
        scale, used = C.c_double(0), C.c_int32(0)
        f = self._lib.orbx_estimate_scale
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, DP,
                      C.POINTER(C.c_int32)]
        self._chk(f(self._h, _ptr(a), _ptr(va), len(a), _ptr(b), _ptr(vb), len(b), C.byref(scale), C.byref(used)))
        return scale.value, used.value

    def batch_scale_consecutive(self, K):
        """Triangulates and scales every pair of the last batch_pose_consecutive on the device."""
        K, kp = _d(K, (3, 3))
        f = self._lib.orbx_batch_scale_consecutive
        f.argtypes = [C.c_void_p, DP]
        self._chk(f(self._h, kp))
        self._scale_pairs = getattr(self, "_pose_pairs", 0)

    def batch_scale_fetch(self, first=0, n=None):
        """dict of arrays for pairs [first, first + n): scale (float64), triplets, ratios_used (int32)."""
        if n is None:
            n = getattr(self, "_scale_pairs", 0) - first
        m = max(n, 0)  # a negative n (nothing scaled yet) is the C entry's to refuse
        scale, trip, used = np.zeros(m), np.zeros(m, np.int32), np.zeros(m, np.int32)
        f = self._lib.orbx_batch_scale_fetch
        f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(f(self._h, first, n, _ptr(scale), _ptr(trip), _ptr(used)))
        return {"scale": scale, "triplets": trip, "ratios_used": used}

    def batch_points_fetch(self, pair, capacity=None):
        """The triangulated points of one pair in batch_match_fetch order: (xyz (n, 3) float32, valid (n,) uint8).
        capacity=None: sized from the pair's match count."""
        f = self._lib.orbx_batch_points_fetch
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
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

    for f in (triangulate, estimate_scale, batch_scale_consecutive, batch_scale_fetch, batch_points_fetch):
        setattr(Context, f.__name__, f)


_scale_methods()


BA_CONVERGENCE, BA_NO_CONVERGENCE, BA_FAILURE, BA_SKIPPED = range(4)
BA_MAX_POSES = 8


class BaSummary(C.Structure):
    _fields_ = [("termination", C.c_int32), ("iterations", C.c_int32), ("successful_steps", C.c_int32),
                ("reserved", C.c_int32), ("initial_cost", C.c_double), ("final_cost", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k in ("termination", "iterations", "successful_steps", "initial_cost",
                                              "final_cost")}


def _ba_methods():
    """Sliding-window bundle adjustment: the reference's Ceres solve (include/orbx.h)."""
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)

    def _d(a, shape):
        a = np.array(np.asarray(a, np.float64).reshape(shape), order="C")  # a copy: the entry writes in place
        return a, a.ctypes.data_as(DP)

    def _i(a):
        a = np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1))
        return a, a.ctypes.data_as(IP)

    def bundle_adjust(self, K, poses, points, obs_point, obs_pose, obs_xy, huber_delta=1.0, max_iters=200):
        """One window: (poses (W, 6), points (N, 3), summary dict).  poses: angle-axis + translation, world ->
        camera; pose 0 is constant.  The outputs equal the inputs unless the summary says convergence."""
        (K, kp), (poses, pp), (points, xp) = _d(K, (3, 3)), _d(poses, (-1, 6)), _d(points, (-1, 3))
        (op, opp), (oq, oqp), (xy, xyp) = _i(obs_point), _i(obs_pose), _d(obs_xy, (-1, 2))
        if not len(op) == len(oq) == len(xy):
            raise ValueError("obs_point, obs_pose and obs_xy differ in length")
        out = BaSummary()
        f = self._lib.orbx_bundle_adjust
        f.argtypes = [C.c_void_p, DP, C.c_int, DP, C.c_int, DP, C.c_int, IP, IP, DP, C.c_double, C.c_int,
                      C.POINTER(BaSummary)]
        self._chk(f(self._h, kp, len(poses), pp, len(points), xp, len(op), opp, oqp, xyp, huber_delta, max_iters,
                    C.byref(out)))
        return poses, points, out.as_dict()

    def bundle_adjust_batch(self, K, windows, huber_delta=1.0, max_iters=200):
        """Many independent windows in one launch.  windows: a sequence of (poses, points, obs_point, obs_pose,
        obs_xy) with window-local indices; returns a list of (poses, points, summary dict)."""
        n = len(windows)
        cat = lambda k, dt, sh: np.concatenate([np.asarray(w[k], dt).reshape(sh) for w in windows]) if n else np.zeros(sh, dt)
        off = lambda k, sh: np.concatenate([[0], np.cumsum([len(np.asarray(w[k]).reshape(sh)) for w in windows])]).astype(np.int32)
        (K, kp) = _d(K, (3, 3))
        (poses, pp), (points, xp), (xy, xyp) = _d(cat(0, np.float64, (-1, 6)), (-1, 6)), _d(cat(1, np.float64, (-1, 3)), (-1, 3)), _d(cat(4, np.float64, (-1, 2)), (-1, 2))
        (op, opp), (oq, oqp) = _i(cat(2, np.int32, (-1,))), _i(cat(3, np.int32, (-1,)))
        (po, pop), (xo, xop), (oo, oop) = _i(off(0, (-1, 6))), _i(off(1, (-1, 3))), _i(off(2, (-1,)))
        if not len(op) == len(oq) == len(xy):
            raise ValueError("obs_point, obs_pose and obs_xy differ in length")
        out = (BaSummary * max(n, 1))()
        f = self._lib.orbx_bundle_adjust_batch
        f.argtypes = [C.c_void_p, DP, C.c_int, IP, DP, IP, DP, IP, IP, IP, DP, C.c_double, C.c_int,
                      C.POINTER(BaSummary)]
        self._chk(f(self._h, kp, n, pop, pp, xop, xp, oop, opp, oqp, xyp, huber_delta, max_iters, out))
        return [(poses[po[w]:po[w + 1]], points[xo[w]:xo[w + 1]], out[w].as_dict()) for w in range(n)]

    for f in (bundle_adjust, bundle_adjust_batch):
        setattr(Context, f.__name__, f)


_ba_methods()


class GoodFeaturesView(C.Structure):
    _fields_ = [("counts", C.c_void_p), ("corners_xy", C.c_void_p), ("slot_capacity", C.c_int32), ("n", C.c_int32)]


def _gftt_view(a):
    # a row-strided uint8 view (a region of a larger image) is handed over as it is
    if isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.ndim == 2 and a.strides[1] == 1 and \
            a.strides[0] >= a.shape[1]:
        return a
    return _img(a)


def _gftt_methods():
    """Shi-Tomasi corners: cv::goodFeaturesToTrack (include/orbx.h)."""
    _view = _gftt_view

    def corner_min_eigen_val(self, image):
        """cv::cornerMinEigenVal(image, eig, 3, 3): the (h, w) float32 response map."""
        image = _view(image)
        h, w = image.shape
        out = np.zeros((h, w), np.float32)
        f = self._lib.orbx_corner_min_eigen_val
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        self._chk(f(self._h, _ptr(image), w, h, image.strides[0], _ptr(out)))
        return out

    def good_features_to_track(self, image, max_corners=2000, quality_level=0.01, min_distance=8.0, capacity=None):
        """cv::goodFeaturesToTrack(image, corners, maxCorners, qualityLevel, minDistance) as called at
        with_bundle_adjustment.cpp:586-593: (n, 2) float32 corners (x, y), strongest first.  max_corners <= 0: no
        limit.  capacity=None: sized for the call (max_corners, or every interior pixel)."""
        image = _view(image)
        h, w = image.shape
        if capacity is None:
            capacity = max_corners if max_corners > 0 else max((w - 2) * (h - 2), 1)
        out = np.zeros((max(capacity, 1), 2), np.float32)
        cnt = C.c_int(0)
        f = self._lib.orbx_good_features_to_track
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p,
                      C.c_int, C.POINTER(C.c_int)]
        self._chk(f(self._h, _ptr(image), w, h, image.strides[0], max_corners, quality_level, min_distance, _ptr(out),
                    capacity, C.byref(cnt)))
        return out[:cnt.value].copy()

    def good_features_batch(self, frames, max_corners=2000, quality_level=0.01, min_distance=8.0, stream=None):
        """orbx_good_features_batch_device on (n, h, w) uint8 frames: a torch device tensor (any strides with unit
        pixel stride; the caller has synchronised its producer, or passes the producer's stream) or a numpy array
        (copied to the device first).  Asynchronous; good_features_fetch delivers the results."""
        import torch

        if isinstance(frames, np.ndarray):
            frames = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.uint8)).cuda()
            torch.cuda.synchronize()
        if frames.dtype != torch.uint8 or frames.dim() != 3 or not frames.is_cuda or frames.stride(2) != 1:
            raise ValueError("frames must be (n, h, w) uint8 on the device with unit pixel stride")
        self._gf_frames = frames  # kept alive until the next batch
        n, h, w = frames.shape
        rs = frames.stride(1)
        fs = max(frames.stride(0), rs * (h - 1) + w) if n == 1 else frames.stride(0)
        f = self._lib.orbx_good_features_batch_device
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_double,
                      C.c_double, C.c_void_p]
        self._chk(f(self._h, C.c_void_p(frames.data_ptr()), n, w, h, rs, fs, max_corners, quality_level,
                    min_distance, C.c_void_p(stream) if stream else None))

    def good_features_view(self):
        """The device-side result block of the last good-features batch (orbx_good_features_results_device)."""
        v = GoodFeaturesView()
        self._chk(self._lib.orbx_good_features_results_device(self._h, C.byref(v)))
        return v

    def good_features_fetch(self, first=0, n=None):
        """Results of frames [first, first + n) of the last good-features batch: a list of (count, 2) float32 arrays."""
        v = self.good_features_view()
        if n is None:
            n = v.n - first
        counts = np.zeros(max(n, 1), np.int32)
        xy = np.zeros((max(n, 1), v.slot_capacity, 2), np.float32)
        f = self._lib.orbx_good_features_fetch
        f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        self._chk(f(self._h, first, n, _ptr(counts), _ptr(xy)))
        return [xy[i, :counts[i]].copy() for i in range(n)]

    def good_features_workspace_limit(self, nbytes):
        """Bound of the good-features workspace in bytes (0: the default); a larger batch runs in slices."""
        f = self._lib.orbx_good_features_workspace_limit
        f.argtypes = [C.c_void_p, C.c_size_t]
        self._chk(f(self._h, nbytes))

    for f in (corner_min_eigen_val, good_features_to_track, good_features_batch, good_features_view,
              good_features_fetch, good_features_workspace_limit):
        setattr(Context, f.__name__, f)


_gftt_methods()


class GoodFeaturesTopupView(C.Structure):
    _fields_ = [("counts", C.c_void_p), ("carried", C.c_void_p), ("points_xy", C.c_void_p), ("origin", C.c_void_p),
                ("slot_capacity", C.c_int32), ("n", C.c_int32)]


def _gftt_topup_methods():
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
        import torch

        uploaded = any(isinstance(a, np.ndarray) for a in (frames, seeds, seen))
        if isinstance(frames, np.ndarray):
            frames = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.uint8)).cuda()
        if frames.dtype != torch.uint8 or frames.dim() != 3 or not frames.is_cuda or frames.stride(2) != 1:
            raise ValueError("frames must be (n, h, w) uint8 on the device with unit pixel stride")
        n, h, w = frames.shape
        if isinstance(seeds, np.ndarray):
            seeds = torch.from_numpy(np.ascontiguousarray(seeds, np.float32)).cuda()
        if isinstance(seen, np.ndarray):
            seen = torch.from_numpy(np.ascontiguousarray(seen, np.int32)).cuda()
        keep = [frames]
        if torch.is_tensor(seeds):
            if seeds.dtype != torch.float32 or not seeds.is_cuda or not seeds.is_contiguous() or seeds.dim() != 3 or \
                    seeds.shape[0] != n or seeds.shape[2] != 2:
                raise ValueError("seeds must be (n, seed_capacity, 2) float32, contiguous, on the device")
            seed_capacity, seed_point_stride, seed_frame_stride = seeds.shape[1], 2, 2 * seeds.shape[1]
            keep.append(seeds)
            seeds = seeds.data_ptr()
        elif seed_capacity is None or seed_frame_stride is None:
            raise ValueError("a raw seed address needs seed_capacity and seed_frame_stride")
        if torch.is_tensor(seen):
            if seen.dtype != torch.int32 or not seen.is_cuda or not seen.is_contiguous() or \
                    seen.numel() != n * seed_capacity:
                raise ValueError("seen must be (n, seed_capacity) int32, contiguous, on the device")
            keep.append(seen)
            seen = seen.data_ptr()
        if uploaded:
            torch.cuda.synchronize()  # the uploads above ran on torch's stream
        self._gft_keep = keep  # kept alive until the next call
        rs = frames.stride(1)
        fs = max(frames.stride(0), rs * (h - 1) + w) if n == 1 else frames.stride(0)
        f = self._lib.orbx_good_features_topup_device
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t,
                      C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p]
        self._chk(f(self._h, C.c_void_p(frames.data_ptr()), n, w, h, rs, fs, C.c_void_p(seeds), seed_point_stride,
                    seed_frame_stride, C.c_void_p(seen) if seen else None, seen_min, seed_capacity, max_corners,
                    quality_level, min_distance, C.c_void_p(stream) if stream else None))

    def good_features_topup_view(self):
        """The device-side result block of the last top-up (orbx_good_features_topup_results_device)."""
        v = GoodFeaturesTopupView()
        self._chk(self._lib.orbx_good_features_topup_results_device(self._h, C.byref(v)))
        return v

    def good_features_topup_fetch(self, first=0, n=None):
        """Frames [first, first + n) of the last top-up as whole arrays: counts (n,), carried (n,), points
        (n, slot_capacity, 2) float32 and origin (n, slot_capacity) int32 -- zero / -1 at and beyond counts[f]."""
        v = self.good_features_topup_view()
        if n is None:
            n = v.n - first
        m = max(n, 1)
        counts, carried = np.zeros(m, np.int32), np.zeros(m, np.int32)
        points = np.zeros((m, v.slot_capacity, 2), np.float32)
        origin = np.zeros((m, v.slot_capacity), np.int32)
        f = self._lib.orbx_good_features_topup_fetch
        f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(f(self._h, first, n, _ptr(counts), _ptr(carried), _ptr(points), _ptr(origin)))
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
        f = self._lib.orbx_good_features_topup
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double,
                      C.c_double, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        self._chk(f(self._h, _ptr(image), w, h, image.strides[0], _ptr(seeds) if len(seeds) else None, len(seeds),
                    max_corners, quality_level, min_distance, _ptr(points), _ptr(origin), capacity, C.byref(cnt),
                    C.byref(car)))
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
        f = self._lib.orbx_good_features_to_track_masked
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double,
                      C.c_double, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        self._chk(f(self._h, _ptr(image), w, h, image.strides[0], _ptr(mask), mask.strides[0], max_corners,
                    quality_level, min_distance, _ptr(out), capacity, C.byref(cnt)))
        return out[:cnt.value].copy()

    for f in (good_features_topup, good_features_topup_view, good_features_topup_fetch, good_features_topup_one,
              good_features_to_track_masked):
        setattr(Context, f.__name__, f)


_gftt_topup_methods()


class LkWindowsView(C.Structure):
    _fields_ = [("tracks_xy", C.c_void_p), ("seen", C.c_void_p), ("err", C.c_void_p), ("slot_capacity", C.c_int32),
                ("window_len", C.c_int32), ("n_windows", C.c_int32)]


class LkWindowsFbView(C.Structure):
    _fields_ = [("fb_d2", C.c_void_p), ("lost", C.c_void_p), ("slot_capacity", C.c_int32), ("window_len", C.c_int32),
                ("n_windows", C.c_int32)]


LK_FB_ALIVE, LK_FB_FORWARD, LK_FB_BACKWARD, LK_FB_DISTANCE = range(4)  # `lost` of the forward-backward check


def _lk_window_methods():
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
        import torch

        uploaded = any(isinstance(a, np.ndarray) for a in (frames, points, counts))
        if isinstance(frames, np.ndarray):
            frames = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.uint8)).cuda()
        if frames.dtype != torch.uint8 or frames.dim() != 3 or not frames.is_cuda or frames.stride(2) != 1:
            raise ValueError("frames must be (n, h, w) uint8 on the device with unit pixel stride")
        window_first = np.ascontiguousarray(window_first, np.int32).reshape(-1)
        nw = len(window_first)
        if isinstance(points, np.ndarray):
            points = torch.from_numpy(np.ascontiguousarray(points, np.float32)).cuda()
        if isinstance(counts, np.ndarray):
            counts = torch.from_numpy(np.ascontiguousarray(counts, np.int32)).cuda()
        keep = [frames]
        if torch.is_tensor(points):
            if points.dtype != torch.float32 or not points.is_cuda or not points.is_contiguous() or \
                    points.dim() != 3 or points.shape[0] != nw or points.shape[2] != 2:
                raise ValueError("points must be (n_windows, slot_capacity, 2) float32, contiguous, on the device")
            if slot_capacity is None:
                slot_capacity = points.shape[1]
            elif slot_capacity != points.shape[1]:
                raise ValueError("slot_capacity differs from points.shape[1]")
            keep.append(points)
            points = points.data_ptr()
        elif slot_capacity is None:
            raise ValueError("a raw points address needs slot_capacity")
        if torch.is_tensor(counts):
            if counts.dtype != torch.int32 or not counts.is_cuda or not counts.is_contiguous() or counts.numel() != nw:
                raise ValueError("counts must be (n_windows,) int32, contiguous, on the device")
            keep.append(counts)
            counts = counts.data_ptr()
        if uploaded:
            torch.cuda.synchronize()  # the uploads above ran on torch's stream
        self._lkw_keep = keep  # kept alive until the next call
        n, h, w = frames.shape
        rs = frames.stride(1)
        fs = max(frames.stride(0), rs * (h - 1) + w) if n == 1 else frames.stride(0)
        args = [self._h, C.c_void_p(frames.data_ptr()), n, w, h, rs, fs, _ptr(window_first), nw, window_len,
                C.c_void_p(points), C.c_void_p(counts) if counts else None, slot_capacity, win, max_level, max_iters,
                epsilon]
        types = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_int, C.c_int,
                 C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double]
        if fb_threshold is None:
            f = self._lib.orbx_lk_track_windows_device
        else:
            f = self._lib.orbx_lk_track_windows_fb_device
            args.append(fb_threshold)
            types.append(C.c_float)
        f.argtypes = types + [C.c_void_p]
        self._chk(f(*args, C.c_void_p(stream) if stream else None))

    def lk_windows_view(self):
        """The device-side result block of the last windows call (orbx_lk_windows_results_device)."""
        v = LkWindowsView()
        self._chk(self._lib.orbx_lk_windows_results_device(self._h, C.byref(v)))
        return v

    def lk_windows_fetch(self, first=0, n=None):
        """Windows [first, first + n) of the last windows call: tracks (n, slots, window_len, 2) float32, seen
        (n, slots) int32, err (n, slots, window_len - 1) float32, zero past `seen` and in unused slots."""
        v = self.lk_windows_view()
        if n is None:
            n = v.n_windows - first
        m = max(n, 1)
        tracks = np.zeros((m, v.slot_capacity, v.window_len, 2), np.float32)
        seen = np.zeros((m, v.slot_capacity), np.int32)
        err = np.zeros((m, v.slot_capacity, v.window_len - 1), np.float32)
        f = self._lib.orbx_lk_windows_fetch
        f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(f(self._h, first, n, _ptr(tracks), _ptr(seen), _ptr(err)))
        return tracks, seen, err

    def lk_windows_fb_view(self):
        """What the forward-backward check added to the last windows call, on the device
        (orbx_lk_windows_fb_results_device); raises after a call without the check."""
        v = LkWindowsFbView()
        f = self._lib.orbx_lk_windows_fb_results_device
        f.argtypes = [C.c_void_p, C.c_void_p]
        self._chk(f(self._h, C.byref(v)))
        return v

    def lk_windows_fb_fetch(self, first=0, n=None):
        """Windows [first, first + n) of the last windows call with the check: fb_d2 (n, slots, window_len - 1)
        float32, the squared forward-backward distance of every pair that passed, and lost (n, slots) int32, 0 or the
        reason the track ended (LK_FB_FORWARD / LK_FB_BACKWARD / LK_FB_DISTANCE)."""
        v = self.lk_windows_fb_view()
        if n is None:
            n = v.n_windows - first
        m = max(n, 1)
        fb_d2 = np.zeros((m, v.slot_capacity, v.window_len - 1), np.float32)
        lost = np.zeros((m, v.slot_capacity), np.int32)
        f = self._lib.orbx_lk_windows_fb_fetch
        f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        self._chk(f(self._h, first, n, _ptr(fb_d2), _ptr(lost)))
        return fb_d2, lost

    def lk_workspace_limit(self, nbytes):
        """Bound of the windows workspace in bytes (0: the default); more frames run in slices of whole windows."""
        f = self._lib.orbx_lk_workspace_limit
        f.argtypes = [C.c_void_p, C.c_size_t]
        self._chk(f(self._h, nbytes))

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
        types = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_int,
                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double]
        if fb_threshold is None:
            f = self._lib.orbx_lk_track_window
            f.argtypes = types
            self._chk(f(*args))
            return tracks[:n].copy(), seen[:n].copy(), err[:n, :nf - 1].copy()
        fb_d2 = np.zeros_like(err)
        lost = np.zeros(max(n, 1), np.int32)
        f = self._lib.orbx_lk_track_window_fb
        f.argtypes = types + [C.c_float, C.c_void_p, C.c_void_p]
        self._chk(f(*args, fb_threshold, _ptr(fb_d2), _ptr(lost)))
        return tracks[:n].copy(), seen[:n].copy(), err[:n, :nf - 1].copy(), fb_d2[:n, :nf - 1].copy(), lost[:n].copy()

    for f in (lk_track_windows, lk_windows_view, lk_windows_fetch, lk_windows_fb_view, lk_windows_fb_fetch,
              lk_workspace_limit, lk_track_window):
        setattr(Context, f.__name__, f)


_lk_window_methods()


LM_OK, LM_BASELINE, LM_EMPTY, LM_BAD_POSE = range(4)


class LandmarksView(C.Structure):
    _fields_ = [("status", C.c_void_p), ("pose_offset", C.c_void_p), ("point_offset", C.c_void_p),
                ("obs_offset", C.c_void_p), ("points3", C.c_void_p), ("rows", C.c_void_p), ("obs_pose", C.c_void_p),
                ("obs_xy", C.c_void_p), ("slot_of_point", C.c_void_p), ("slot_capacity", C.c_int32),
                ("window_len", C.c_int32), ("n_windows", C.c_int32)]


def _landmark_methods():
    """Landmarks of tracked windows built on the device and bundle-adjusted there:
    buildLandmarksFromFirstTwoFramesAndTracks + the window's solve (include/orbx.h)."""
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)

    def _d(a, shape):
        a = np.array(np.asarray(a, np.float64).reshape(shape), order="C")
        return a, a.ctypes.data_as(DP)

    def landmarks_build(self, K, tracks, seen, poses, n_windows=None, slot_capacity=None, window_len=None,
                        stream=None):
        """orbx_landmarks_build_device.  tracks: (n_windows, slots, window_len, 2) float32 and seen: (n_windows,
        slots) int32, each a torch device tensor, a numpy array (copied to the device first) or a raw device address
        (then n_windows, slot_capacity and window_len are required) -- e.g. the fields of lk_windows_view().  poses:
        host, (n_windows, window_len, 6).  Asynchronous; landmarks_fetch delivers the block."""
        import torch

        uploaded = any(isinstance(a, np.ndarray) for a in (tracks, seen))
        if isinstance(tracks, np.ndarray):
            tracks = torch.from_numpy(np.ascontiguousarray(tracks, np.float32)).cuda()
        if isinstance(seen, np.ndarray):
            seen = torch.from_numpy(np.ascontiguousarray(seen, np.int32)).cuda()
        keep = []
        if torch.is_tensor(tracks):
            if tracks.dtype != torch.float32 or not tracks.is_cuda or not tracks.is_contiguous() or \
                    tracks.dim() != 4 or tracks.shape[3] != 2:
                raise ValueError("tracks must be (n_windows, slots, window_len, 2) float32, contiguous, on the device")
            shape = tuple(tracks.shape[:3])
            if (n_windows, slot_capacity, window_len) not in ((None, None, None), shape):
                raise ValueError("n_windows / slot_capacity / window_len differ from tracks.shape")
            n_windows, slot_capacity, window_len = shape
            keep.append(tracks)
            tracks = tracks.data_ptr()
        elif None in (n_windows, slot_capacity, window_len):
            raise ValueError("a raw tracks address needs n_windows, slot_capacity and window_len")
        if torch.is_tensor(seen):
            if seen.dtype != torch.int32 or not seen.is_cuda or not seen.is_contiguous() or \
                    seen.numel() != n_windows * slot_capacity:
                raise ValueError("seen must be (n_windows, slots) int32, contiguous, on the device")
            keep.append(seen)
            seen = seen.data_ptr()
        if uploaded:
            torch.cuda.synchronize()  # the uploads above ran on torch's stream
        self._lm_keep = keep  # kept alive until the next build
        (K, kp) = _d(K, (3, 3))
        (poses, pp) = _d(poses, (-1, 6))
        if len(poses) != max(n_windows, 0) * max(window_len, 0):
            raise ValueError("poses must be (n_windows, window_len, 6)")
        f = self._lib.orbx_landmarks_build_device
        f.argtypes = [C.c_void_p, DP, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, DP, C.c_void_p]
        self._chk(f(self._h, kp, C.c_void_p(tracks), C.c_void_p(seen), n_windows, slot_capacity, window_len, pp,
                    C.c_void_p(stream) if stream else None))

    def landmarks_view(self):
        """The device-side landmarks block of the last build (orbx_landmarks_results_device)."""
        v = LandmarksView()
        self._chk(self._lib.orbx_landmarks_results_device(self._h, C.byref(v)))
        return v

    def landmarks_fetch(self, first=0, n=None):
        """Windows [first, first + n) of the last build in the format of bundle_adjust_batch: a dict of status (n),
        pose_offset / point_offset / obs_offset (n + 1), points3 (N, 3), slot_of_point (N), obs_point / obs_pose (M)
        and obs_xy (M, 2)."""
        if n is None:
            n = self.landmarks_view().n_windows - first
        f = self._lib.orbx_landmarks_fetch
        f.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 3 + [
            C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
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
        f = self._lib.orbx_bundle_adjust_landmarks_device
        f.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_void_p]
        self._chk(f(self._h, huber_delta, max_iters, C.c_void_p(stream) if stream else None))

    def bundle_adjust_landmarks_fetch(self, first=0, n=None, points=True):
        """Windows [first, first + n) of the last solve: poses (n, window_len, 6), a list of summary dicts, and the
        points (N, 3) in the order of the block (None with points=False)."""
        v = self.landmarks_view()
        if n is None:
            n = v.n_windows - first
        m = max(n, 1)
        poses = np.zeros((m, v.window_len, 6))
        out = (BaSummary * m)()
        f = self._lib.orbx_bundle_adjust_landmarks_fetch
        f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        cnt = C.c_int(0)
        pts = None
        if points:
            self._chk(f(self._h, first, n, None, None, None, 0, C.byref(cnt)))
            pts = np.zeros((cnt.value, 3))
        self._chk(f(self._h, first, n, _ptr(poses), C.cast(out, C.c_void_p), _ptr(pts) if points and pts.size else None,
                    cnt.value, C.byref(cnt)))
        return poses[:n], [out[w].as_dict() for w in range(n)], pts

    def bundle_adjust_tracks(self, K, tracks, seen, poses, huber_delta=1.0, max_iters=200):
        """orbx_bundle_adjust_tracks: one window of host tracks (slots, window_len, 2), seen (slots) and poses
        (window_len, 6) through both stages.  Returns (poses, summary dict, landmarks status, points (N, 3),
        slot_of_point (N))."""
        tracks = np.ascontiguousarray(tracks, np.float32)
        if tracks.ndim != 3 or tracks.shape[2] != 2:
            raise ValueError("tracks must be (slots, window_len, 2) float32")
        slots, wl = tracks.shape[:2]
        seen = np.ascontiguousarray(seen, np.int32).reshape(-1)
        if len(seen) != slots:
            raise ValueError("seen must have one entry per slot")
        (K, kp) = _d(K, (3, 3))
        (poses, pp) = _d(poses, (-1, 6))
        if len(poses) != wl:
            raise ValueError("poses must be (window_len, 6)")
        pts = np.zeros((max(slots, 1), 3))
        sop = np.zeros(max(slots, 1), np.int32)
        st, cnt, out = C.c_int32(-1), C.c_int(0), BaSummary()
        f = self._lib.orbx_bundle_adjust_tracks
        f.argtypes = [C.c_void_p, DP, C.c_void_p, C.c_void_p, C.c_int, C.c_int, DP, C.c_double, C.c_int,
                      C.POINTER(C.c_int32), C.POINTER(BaSummary), C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        self._chk(f(self._h, kp, _ptr(tracks), _ptr(seen), slots, wl, pp, huber_delta, max_iters, C.byref(st),
                    C.byref(out), _ptr(pts), _ptr(sop), slots, C.byref(cnt)))
        return poses, out.as_dict(), st.value, pts[:cnt.value].copy(), sop[:cnt.value].copy()

    for f in (landmarks_build, landmarks_view, landmarks_fetch, bundle_adjust_landmarks,
              bundle_adjust_landmarks_fetch, bundle_adjust_tracks):
        setattr(Context, f.__name__, f)


_landmark_methods()


class TracksPoseView(C.Structure):
    _fields_ = [("pose", C.c_void_p), ("n", C.c_void_p), ("scale", C.c_void_p), ("slot_of", C.c_void_p),
                ("mask", C.c_void_p), ("xyz", C.c_void_p), ("valid", C.c_void_p), ("slot_capacity", C.c_int32),
                ("window_len", C.c_int32), ("n_windows", C.c_int32), ("n_pairs", C.c_int32)]


def _tracks_pose_methods():
    """Pose, triangulated points and relative scale of every consecutive frame pair of tracked windows, from the
    tracks block on the device (include/orbx.h)."""
    DP = C.POINTER(C.c_double)

    def _K(K):
        K = np.ascontiguousarray(np.asarray(K, np.float64).reshape(3, 3))
        return K, K.ctypes.data_as(DP)

    def tracks_pose(self, K, tracks, seen=None, n_windows=None, slot_capacity=None, window_len=None, prob=0.999,
                    threshold=1.0, max_iters=1000, seed=0, stream=None):
        """orbx_tracks_pose_device.  tracks: an LkWindowsView (lk_windows_view(); seen and the three sizes come from
        it), or (n_windows, slots, window_len, 2) float32 with seen (n_windows, slots) int32, each a torch device
        tensor, a numpy array (copied to the device first) or a raw device address (then n_windows, slot_capacity and
        window_len are required).  Asynchronous; tracks_pose_fetch / tracks_pose_pair_fetch deliver the block."""
        import torch

        if isinstance(tracks, LkWindowsView):
            v = tracks
            tracks, seen = v.tracks_xy, v.seen
            n_windows, slot_capacity, window_len = v.n_windows, v.slot_capacity, v.window_len
        uploaded = any(isinstance(a, np.ndarray) for a in (tracks, seen))
        if isinstance(tracks, np.ndarray):
            tracks = torch.from_numpy(np.ascontiguousarray(tracks, np.float32)).cuda()
        if isinstance(seen, np.ndarray):
            seen = torch.from_numpy(np.ascontiguousarray(seen, np.int32)).cuda()
        keep = []
        if torch.is_tensor(tracks):
            if tracks.dtype != torch.float32 or not tracks.is_cuda or not tracks.is_contiguous() or \
                    tracks.dim() != 4 or tracks.shape[3] != 2:
                raise ValueError("tracks must be (n_windows, slots, window_len, 2) float32, contiguous, on the device")
            shape = tuple(tracks.shape[:3])
            if (n_windows, slot_capacity, window_len) not in ((None, None, None), shape):
                raise ValueError("n_windows / slot_capacity / window_len differ from tracks.shape")
            n_windows, slot_capacity, window_len = shape
            keep.append(tracks)
            tracks = tracks.data_ptr()
        elif None in (n_windows, slot_capacity, window_len):
            raise ValueError("a raw tracks address needs n_windows, slot_capacity and window_len")
        if torch.is_tensor(seen):
            if seen.dtype != torch.int32 or not seen.is_cuda or not seen.is_contiguous() or \
                    seen.numel() != n_windows * slot_capacity:
                raise ValueError("seen must be (n_windows, slots) int32, contiguous, on the device")
            keep.append(seen)
            seen = seen.data_ptr()
        if uploaded:
            torch.cuda.synchronize()  # the uploads above ran on torch's stream
        self._tp_keep = keep  # kept alive until the next call
        K, kp = _K(K)
        f = self._lib.orbx_tracks_pose_device
        f.argtypes = [C.c_void_p, DP, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                      C.c_int, C.c_uint64, C.c_void_p]
        self._chk(f(self._h, kp, C.c_void_p(tracks), C.c_void_p(seen), n_windows, slot_capacity, window_len, prob,
                    threshold, max_iters, seed, C.c_void_p(stream) if stream else None))

    def tracks_pose_view(self):
        """The device-side block of the last tracks_pose (orbx_tracks_pose_results_device)."""
        v = TracksPoseView()
        self._chk(self._lib.orbx_tracks_pose_results_device(self._h, C.byref(v)))
        return v

    def _fetch_arrays(m):
        return dict(E=np.zeros((m, 3, 3)), R=np.zeros((m, 3, 3)), t=np.zeros((m, 3)), inliers=np.zeros(m, np.int32),
                    good=np.zeros(m, np.int32), iters=np.zeros(m, np.int32), n=np.zeros(m, np.int32),
                    scale=np.zeros(m), triplets=np.zeros(m, np.int32), ratios_used=np.zeros(m, np.int32))

    _ORDER = ("E", "R", "t", "inliers", "good", "iters", "n", "scale", "triplets", "ratios_used")

    def tracks_pose_fetch(self, first=0, n=None):
        """Pairs [first, first + n) of the last tracks_pose (pair p = w * (window_len - 1) + k): dict of E, R
        (n, 3, 3), t (n, 3), inliers, good, iters, n (the list lengths), scale, triplets, ratios_used."""
        if n is None:
            n = self.tracks_pose_view().n_pairs - first
        out = _fetch_arrays(max(n, 0))
        f = self._lib.orbx_tracks_pose_fetch
        f.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 10
        self._chk(f(self._h, first, n, *[_ptr(out[k]) for k in _ORDER]))
        return out

    def tracks_pose_pair_fetch(self, pair, capacity=None):
        """The lists of one pair, one entry per surviving slot in ascending slot order: dict of slot_of (n,) int32,
        mask (n,) uint8, xyz (n, 3) float32, valid (n,) uint8.  capacity=None: sized from the pair's count."""
        f = self._lib.orbx_tracks_pose_pair_fetch
        f.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.POINTER(C.c_int)]
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
        tracks = np.ascontiguousarray(tracks, np.float32)
        if tracks.ndim != 3 or tracks.shape[2] != 2:
            raise ValueError("tracks must be (slots, window_len, 2) float32")
        slots, wl = tracks.shape[:2]
        seen = np.ascontiguousarray(seen, np.int32).reshape(-1)
        if len(seen) != slots:
            raise ValueError("seen must have one entry per slot")
        K, kp = _K(K)
        out = _fetch_arrays(max(wl - 1, 0))
        f = self._lib.orbx_tracks_pose
        f.argtypes = [C.c_void_p, DP, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                      C.c_uint64] + [C.c_void_p] * 10
        self._chk(f(self._h, kp, _ptr(tracks), _ptr(seen), slots, wl, prob, threshold, max_iters, seed,
                    *[_ptr(out[k]) for k in _ORDER]))
        return out

    for f in (tracks_pose, tracks_pose_view, tracks_pose_fetch, tracks_pose_pair_fetch, tracks_pose_window):
        setattr(Context, f.__name__, f)


_tracks_pose_methods()


def chain_trajectory(T0, R, t, scale):
    """cur_pose = cur_pose * T.inv(), T = [R | scale * t], over n relative motions (feature_matching.cpp:77-82):
    (n + 1, 4, 4) poses with poses[0] = T0.  Host only."""
    DP = C.POINTER(C.c_double)
    T0 = np.ascontiguousarray(np.asarray(T0, np.float64).reshape(4, 4))
    R = np.ascontiguousarray(np.asarray(R, np.float64).reshape(-1, 3, 3))
    t = np.ascontiguousarray(np.asarray(t, np.float64).reshape(-1, 3))
    scale = np.ascontiguousarray(np.asarray(scale, np.float64).reshape(-1))
    n = len(R)
    if len(t) != n or len(scale) != n:
        raise ValueError("R, t and scale differ in length")
    poses = np.zeros((n + 1, 4, 4))
    f = load().orbx_chain_trajectory
    f.argtypes = [DP, DP, DP, DP, C.c_int, DP]
    st = f(T0.ctypes.data_as(DP), R.ctypes.data_as(DP), t.ctypes.data_as(DP), scale.ctypes.data_as(DP), n,
           poses.ctypes.data_as(DP))
    if st != OK:
        raise OrbxError(st, "orbx_chain_trajectory")
    return poses


def gaussian_kernel(K, sigma=-1.0):
    out = np.zeros(K * K, np.float32)
    st = load().orbx_gaussian_kernel(K, C.c_float(sigma), _ptr(out))
    if st != OK:
        raise OrbxError(st, "orbx_gaussian_kernel")
    return out.reshape(K, K)


def version():
    return load().orbx_version().decode()
