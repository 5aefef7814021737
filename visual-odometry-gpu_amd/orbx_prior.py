"""ctypes binding of include/orbx_prior.h, the eighth public header of liborbx.so: landmark
priors in the window solve -- the two host entries, the priors of a carried window gathered on the device, and the
solve of the landmarks block with them.  The functions take a Context of `orbx`; the library is the one orbx.load()
returns, and this module's own prototype table is applied to it once (tests/test_orbx_prior_abi.py checks it against
the header)."""
import ctypes as C

import numpy as np

from . import orbx
from .orbx import BaSummary, _count, _dp, _f64, _i32, _ip, _observations, _ptr, _stream

PRIOR_START_GIVEN, PRIOR_START_ANCHOR = range(2)

P, I, D = orbx.P, orbx.I, orbx.D
PROTOTYPES = {
    "orbx_bundle_adjust_prior": (I, [P, P, I, P, I, P, I, P, P, P, P, P, I, D, I, P]),
    "orbx_bundle_adjust_prior_batch": (I, [P, P, I] + [P] * 10 + [I, D, I, P]),
    "orbx_landmarks_priors_carried_device": (I, [P, D, P]),
    "orbx_landmarks_priors_results_device": (I, [P, P]),
    "orbx_landmarks_priors_fetch": (I, [P, I, I, P, P, P, I, P]),
    "orbx_bundle_adjust_landmarks_prior_device": (I, [P, D, I, I, P]),
}
EXPORTS = list(PROTOTYPES)  # every symbol include/orbx_prior.h declares


class LandmarksPriorsView(C.Structure):
    _fields_ = [("prior", C.c_void_p), ("count", C.c_void_p), ("n_windows", C.c_int32)]


_lib = None


def load():
    """The library of orbx.load() with every prototype of PROTOTYPES declared."""
    global _lib
    if _lib is None:
        lib = orbx.load()
        for name, (restype, argtypes) in PROTOTYPES.items():
            f = getattr(lib, name, None)  # (a symbol the library lacks is tests/test_orbx_prior_abi.py's to report)
            if f is not None:
                f.restype = restype
                f.argtypes = argtypes
        _lib = lib
    return _lib


def _priors(prior_xyz, prior_weight, n_points):
    """(xyz (n, 3), weight (n)) as the entries take them, or (None, None): no priors.  Exactly one of them None goes
    to the library as it is, which refuses it."""
    xyz = None if prior_xyz is None else _f64(prior_xyz, (-1, 3))
    wt = None if prior_weight is None else _f64(prior_weight, (-1,))
    for a, what in ((xyz, "prior_xyz"), (wt, "prior_weight")):
        if a is not None and len(a) != n_points:
            raise ValueError("%s and points differ in length" % what)
    return xyz, wt


def bundle_adjust_prior(ctx, K, poses, points, obs_point, obs_pose, obs_xy, prior_xyz=None, prior_weight=None,
                        start=PRIOR_START_GIVEN, huber_delta=1.0, max_iters=200):
    """orbx_bundle_adjust_prior: Context.bundle_adjust with an anchor prior_xyz (N, 3) and a weight prior_weight (N)
    per landmark (both None: no priors).  Returns (poses (W, 6), points (N, 3), summary dict); the outputs equal the
    inputs unless the summary says convergence."""
    K, poses, points = _f64(K, (3, 3)), _f64(poses, (-1, 6), copy=True), _f64(points, (-1, 3), copy=True)
    op, oq, xy = _observations(obs_point, obs_pose, obs_xy)
    pa, pw = _priors(prior_xyz, prior_weight, len(points))
    out = BaSummary()
    ctx._chk(load().orbx_bundle_adjust_prior(ctx._h, _dp(K), len(poses), _dp(poses), len(points), _dp(points), len(op),
                                             _ip(op), _ip(oq), _dp(xy), _ptr(pa), _ptr(pw), start, huber_delta,
                                             max_iters, C.byref(out)))
    return poses, points, out.as_dict()


def bundle_adjust_prior_batch(ctx, K, windows, priors=None, start=PRIOR_START_GIVEN, huber_delta=1.0, max_iters=200):
    """orbx_bundle_adjust_prior_batch: Context.bundle_adjust_batch with priors, a sequence of (prior_xyz, prior_weight)
    per window, or None: no priors.  Returns a list of (poses, points, summary dict)."""
    n = len(windows)
    cat = lambda k, dt, sh: np.concatenate([np.asarray(w[k], dt).reshape(sh) for w in windows]) if n else np.zeros(sh, dt)
    off = lambda k, sh: _i32(np.concatenate([[0], np.cumsum([len(np.asarray(w[k]).reshape(sh)) for w in windows])]))
    K = _f64(K, (3, 3))
    poses, points = _f64(cat(0, np.float64, (-1, 6)), (-1, 6), copy=True), _f64(cat(1, np.float64, (-1, 3)), (-1, 3), copy=True)
    op, oq, xy = _observations(cat(2, np.int32, (-1,)), cat(3, np.int32, (-1,)), cat(4, np.float64, (-1, 2)))
    po, xo, oo = off(0, (-1, 6)), off(1, (-1, 3)), off(2, (-1,))
    pa = pw = None
    if priors is not None:
        if len(priors) != n:
            raise ValueError("priors and windows differ in length")
        pa = np.concatenate([np.asarray(p[0], np.float64).reshape(-1, 3) for p in priors]) if n else np.zeros((0, 3))
        pw = np.concatenate([np.asarray(p[1], np.float64).reshape(-1) for p in priors]) if n else np.zeros(0)
        pa, pw = _priors(pa, pw, len(points))
    out = (BaSummary * max(n, 1))()
    ctx._chk(load().orbx_bundle_adjust_prior_batch(ctx._h, _dp(K), n, _ip(po), _dp(poses), _ip(xo), _dp(points),
                                                   _ip(oo), _ip(op), _ip(oq), _dp(xy), _ptr(pa), _ptr(pw), start,
                                                   huber_delta, max_iters, out))
    return [(poses[po[w]:po[w + 1]], points[xo[w]:xo[w + 1]], out[w].as_dict()) for w in range(n)]


def landmarks_priors_carried(ctx, weight, stream=None):
    """orbx_landmarks_priors_carried_device: rule P6 on the current landmarks block and the last carry block, one
    weight for every carried landmark.  Asynchronous; landmarks_priors_fetch delivers the block."""
    ctx._chk(load().orbx_landmarks_priors_carried_device(ctx._h, weight, _stream(stream)))


def landmarks_priors_view(ctx):
    """The device-side block of the last landmarks_priors_carried (orbx_landmarks_priors_results_device)."""
    v = LandmarksPriorsView()
    ctx._chk(load().orbx_landmarks_priors_results_device(ctx._h, C.byref(v)))
    return v


def landmarks_priors_fetch(ctx, first=0, n=None):
    """Windows [first, first + n) of the last landmarks_priors_carried: a dict of prior_xyz (points, 3), prior_weight
    (points) in the landmarks block's point order, and count (n) int32."""
    v = landmarks_priors_view(ctx)
    n = _count(n, first, v.n_windows)
    f = load().orbx_landmarks_priors_fetch
    cnt, count = C.c_int(0), np.zeros(max(n, 1), np.int32)
    ctx._chk(f(ctx._h, first, n, None, None, _ptr(count), 0, C.byref(cnt)))
    xyz, wt = np.zeros((max(cnt.value, 1), 3)), np.zeros(max(cnt.value, 1))
    ctx._chk(f(ctx._h, first, n, _ptr(xyz), _ptr(wt), None, cnt.value, None))
    return dict(prior_xyz=xyz[:cnt.value], prior_weight=wt[:cnt.value], count=count[:n])


def bundle_adjust_landmarks_prior(ctx, huber_delta=1.0, max_iters=200, start=PRIOR_START_GIVEN, stream=None):
    """orbx_bundle_adjust_landmarks_prior_device: Context.bundle_adjust_landmarks with the last priors block.
    Asynchronous; Context.bundle_adjust_landmarks_fetch delivers the result."""
    ctx._chk(load().orbx_bundle_adjust_landmarks_prior_device(ctx._h, huber_delta, max_iters, start, _stream(stream)))
