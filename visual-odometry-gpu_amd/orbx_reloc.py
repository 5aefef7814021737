"""ctypes binding of include/orbx_reloc.h, the seventh public header of liborbx.so: ORB
descriptors at points the caller already holds, in two banks, and two described point sets joined by descriptor into
the `origin` block that orbx_carry.landmarks_carry reads.  The functions take a Context of `orbx`; the library is the
one orbx.load() returns, and this module's own prototype table is applied to it once (tests/test_orbx_reloc_abi.py
checks it against the header)."""
import ctypes as C

import numpy as np

from . import orbx
from .orbx import _count, _desc, _device_arg, _frames_arg, _gftt_view, _i32, _ip, _ptr, _stream, _sync_uploads

PD_NONE, PD_BORDER, PD_OK = range(3)
PD_BANKS = 2
PD_WORKSPACE_DEFAULT = 512 << 20

P, I, Z, D = orbx.P, orbx.I, orbx.Z, orbx.D
PROTOTYPES = {
    "orbx_describe_points_device": (I, [P, P, I, I, I, I, Z, P, Z, Z, P, I, P, I, I, P]),
    "orbx_describe_points_workspace_limit": (I, [P, Z]),
    "orbx_point_descriptors_results_device": (I, [P, I, P]),
    "orbx_point_descriptors_fetch": (I, [P, I, I, I, P, P, P, P]),
    "orbx_describe_points": (I, [P, P, I, I, I, P, I, P, P, P]),
    "orbx_reassociate_device": (I, [P, P, P, I, P, P, I, I, D, I, I, P]),
    "orbx_reassociate_results_device": (I, [P, P]),
    "orbx_reassociate_fetch": (I, [P, I, I, P, P, P]),
    "orbx_reassociate": (I, [P, P, P, I, P, P, I, D, I, I, P, P, P]),
}
EXPORTS = list(PROTOTYPES)  # every symbol include/orbx_reloc.h declares


class PointDescriptorsView(C.Structure):
    _fields_ = [("desc", C.c_void_p), ("angle", C.c_void_p), ("state", C.c_void_p), ("n_ok", C.c_void_p),
                ("slot_capacity", C.c_int32), ("n", C.c_int32)]


class ReassociateView(C.Structure):
    _fields_ = [("origin", C.c_void_p), ("dist", C.c_void_p), ("count", C.c_void_p), ("q_capacity", C.c_int32),
                ("t_capacity", C.c_int32), ("n_windows", C.c_int32)]


_lib = None


def load():
    """The library of orbx.load() with every prototype of PROTOTYPES declared."""
    global _lib
    if _lib is None:
        lib = orbx.load()
        for name, (restype, argtypes) in PROTOTYPES.items():
            f = getattr(lib, name, None)  # (a symbol the library lacks is tests/test_orbx_reloc_abi.py's to report)
            if f is not None:
                f.restype = restype
                f.argtypes = argtypes
        _lib = lib
    return _lib


def _points_arg(points, n, slot_capacity, point_stride, frame_stride, keep):
    """The point source of describe_points: an (n, slots, 2) float32 torch device tensor with unit stride along the
    pair -- contiguous, or a view such as frame k of an LK tracks block, tracks[:, :, k] -- a numpy array (copied to
    the device) or a raw device address (then with slot_capacity and both strides, in floats): (address,
    slot_capacity, point_stride, frame_stride, whether it was uploaded)."""
    import torch

    uploaded = isinstance(points, np.ndarray)
    if uploaded:
        points = torch.from_numpy(np.ascontiguousarray(points, np.float32)).cuda()
    if not torch.is_tensor(points):
        if None in (slot_capacity, point_stride, frame_stride):
            raise ValueError("a raw points address needs slot_capacity, point_stride and frame_stride")
        return points, slot_capacity, point_stride, frame_stride, False
    if points.dtype != torch.float32 or not points.is_cuda or points.dim() != 3 or points.shape[0] != n or \
            points.shape[2] != 2 or points.stride(2) != 1:
        raise ValueError("points must be (n, slots, 2) float32 on the device with unit stride along the pair")
    if slot_capacity not in (None, points.shape[1]):
        raise ValueError("slot_capacity differs from points.shape[1]")
    keep.append(points)
    cap = points.shape[1]
    ps = points.stride(1) if cap > 1 else 2
    fs = points.stride(0) if n > 1 else max(points.stride(0), ps * (cap - 1) + 2)
    return points.data_ptr(), cap, ps, fs, uploaded


def describe_points(ctx, frames, points, bank=0, seen=None, seen_min=0, counts=None, slot_capacity=None,
                    point_stride=None, frame_stride=None, stream=None):
    """orbx_describe_points_device: rules A-E for the (n, h, w) uint8 frames (Context.good_features_batch's argument)
    at `points` (see _points_arg), with seen (n, slots) int32 and counts (n) int32 as torch device tensors, numpy
    arrays or raw addresses, into `bank`.  Asynchronous; point_descriptors_fetch delivers the block."""
    keep = []
    t, n, h, w, rs, fs, up_f = _frames_arg(frames)
    keep.append(t)
    xy, cap, ps, pfs, up_p = _points_arg(points, n, slot_capacity, point_stride, frame_stride, keep)
    seen, _, up_s = _device_arg(seen, np.int32, lambda a: a.numel() == n * cap,
                                "seen must be (n, slots) int32, contiguous, on the device", keep)
    counts, _, up_c = _device_arg(counts, np.int32, lambda a: a.numel() == n,
                                  "counts must be (n) int32, contiguous, on the device", keep)
    _sync_uploads(up_f, up_p, up_s, up_c)
    if not hasattr(ctx, "_pd_keep"):
        ctx._pd_keep = {}
    ctx._pd_keep[bank] = keep  # (the tensors: kept alive until the next call naming the bank)
    ctx._chk(load().orbx_describe_points_device(ctx._h, t.data_ptr(), n, w, h, rs, fs, xy, ps, pfs, seen, seen_min,
                                                counts, cap, bank, _stream(stream)))


def describe_points_workspace_limit(ctx, nbytes):
    """orbx_describe_points_workspace_limit (0: the default)."""
    ctx._chk(load().orbx_describe_points_workspace_limit(ctx._h, nbytes))


def point_descriptors_view(ctx, bank=0):
    """The device-side block of a bank (orbx_point_descriptors_results_device)."""
    v = PointDescriptorsView()
    ctx._chk(load().orbx_point_descriptors_results_device(ctx._h, bank, C.byref(v)))
    return v


def point_descriptors_fetch(ctx, bank=0, first=0, n=None):
    """Frames [first, first + n) of a bank: a dict of desc (n, slots, 32) uint8, angle (n, slots) float32, state
    (n, slots) int32 and n_ok (n) int32."""
    v = point_descriptors_view(ctx, bank)
    n = _count(n, first, v.n)
    m = max(n, 1)
    desc, angle = np.zeros((m, v.slot_capacity, 32), np.uint8), np.zeros((m, v.slot_capacity), np.float32)
    state, n_ok = np.zeros((m, v.slot_capacity), np.int32), np.zeros(m, np.int32)
    ctx._chk(load().orbx_point_descriptors_fetch(ctx._h, bank, first, n, _ptr(desc), _ptr(angle), _ptr(state),
                                                 _ptr(n_ok)))
    return dict(desc=desc[:n], angle=angle[:n], state=state[:n], n_ok=n_ok[:n])


def describe_points_host(ctx, image, points):
    """orbx_describe_points: one host image and (n, 2) host points.  Returns a dict of angle (n), desc (n, 32) and
    state (n); it runs as a batch of one frame in bank 0."""
    image = _gftt_view(image)
    pts = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 2))
    n = len(pts)
    m = max(n, 1)
    angle, desc, state = np.zeros(m, np.float32), np.zeros((m, 32), np.uint8), np.zeros(m, np.int32)
    h, w = image.shape
    ctx._chk(load().orbx_describe_points(ctx._h, _ptr(image), w, h, image.strides[0], _ptr(pts) if n else None, n,
                                         _ptr(angle), _ptr(desc), _ptr(state)))
    return dict(angle=angle[:n], desc=desc[:n], state=state[:n])


def _set_arg(desc, state, n_windows, capacity, what, keep):
    """One side of reassociate: a PointDescriptorsView, or desc (n_windows, slots, 32) uint8 and state
    (n_windows, slots) int32 as torch device tensors, numpy arrays (copied to the device) or raw addresses (then with
    the sizes): (desc address, state address, n_windows, capacity, whether anything was uploaded)."""
    if isinstance(desc, PointDescriptorsView):
        return desc.desc, desc.state, desc.n, desc.slot_capacity, False
    desc, t, up_d = _device_arg(desc, np.uint8, lambda a: a.dim() == 3 and a.shape[2] == 32,
                                what + " desc must be (n_windows, slots, 32) uint8, contiguous, on the device", keep)
    if t is None:
        if None in (n_windows, capacity):
            raise ValueError("a raw %s address needs n_windows and its capacity" % what)
    else:
        if (n_windows, capacity) not in ((None, None), (t.shape[0], None), tuple(t.shape[:2])):
            raise ValueError("n_windows / capacity differ from the %s desc's shape" % what)
        n_windows, capacity = t.shape[:2]
    state, _, up_s = _device_arg(state, np.int32, lambda a: a.numel() == n_windows * capacity,
                                 what + " state must be (n_windows, slots) int32, contiguous, on the device", keep)
    return desc, state, n_windows, capacity, up_d or up_s


def reassociate(ctx, query_desc, query_state=None, train_desc=None, train_state=None, ratio=0.8, max_distance=256,
                unique=1, n_windows=None, q_capacity=None, t_capacity=None, stream=None):
    """orbx_reassociate_device: rules F-J for n_windows (query, train) pairs of described sets (see _set_arg; a
    view brings its state and sizes).  Asynchronous; reassociate_fetch delivers the block, and reassociate_view's
    origin is what orbx_carry.landmarks_carry takes."""
    keep = []
    qd, qs, nq, qcap, up_q = _set_arg(query_desc, query_state, n_windows, q_capacity, "query", keep)
    td, ts, nt, tcap, up_t = _set_arg(train_desc, train_state, nq, t_capacity, "train", keep)
    if nq != nt:
        raise ValueError("query and train differ in n_windows")
    _sync_uploads(up_q, up_t)
    ctx._ra_keep = keep  # (the tensors: kept alive until the next re-association)
    ctx._chk(load().orbx_reassociate_device(ctx._h, qd, qs, qcap, td, ts, tcap, nq, ratio, max_distance, int(unique),
                                            _stream(stream)))


def reassociate_view(ctx):
    """The device-side block of the last reassociate (orbx_reassociate_results_device)."""
    v = ReassociateView()
    ctx._chk(load().orbx_reassociate_results_device(ctx._h, C.byref(v)))
    return v


def reassociate_fetch(ctx, first=0, n=None):
    """Windows [first, first + n) of the last reassociate: a dict of origin, dist (n, q_capacity) int32 and count (n)
    int32."""
    v = reassociate_view(ctx)
    n = _count(n, first, v.n_windows)
    m = max(n, 1)
    origin, dist = np.zeros((m, v.q_capacity), np.int32), np.zeros((m, v.q_capacity), np.int32)
    count = np.zeros(m, np.int32)
    ctx._chk(load().orbx_reassociate_fetch(ctx._h, first, n, _ptr(origin), _ptr(dist), _ptr(count)))
    return dict(origin=origin[:n], dist=dist[:n], count=count[:n])


def reassociate_host(ctx, query_desc, query_state, train_desc, train_state, ratio=0.8, max_distance=256, unique=1):
    """orbx_reassociate: one window on host arrays.  Returns a dict of origin, dist (nq) and count."""
    qd, td, qs, ts = _desc(query_desc), _desc(train_desc), _i32(query_state), _i32(train_state)
    if len(qd) != len(qs) or len(td) != len(ts):
        raise ValueError("a desc and its state differ in length")
    nq, nt = len(qd), len(td)
    m = max(nq, 1)
    origin, dist, count = np.zeros(m, np.int32), np.zeros(m, np.int32), C.c_int32(-1)
    ctx._chk(load().orbx_reassociate(ctx._h, _ptr(qd) if nq else None, _ip(qs) if nq else None, nq,
                                     _ptr(td) if nt else None, _ip(ts) if nt else None, nt, ratio, max_distance,
                                     int(unique), _ptr(origin), _ptr(dist), C.byref(count)))
    return dict(origin=origin[:nq], dist=dist[:nq], count=count.value)
