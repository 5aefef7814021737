"""Seeded random draws for the side paths: the Hamming matcher, relative pose, triangulation and scale, bundle
adjustment, the Shi-Tomasi entries (batch, top-up, mask), tracks pose -> window-pose chain -> stitch, and the
landmark builds with their solve and write-back gate.

draw(family, seed, index) returns one valid call and its expected result from (family, seed, index) alone: the
generator of every draw is np.random.default_rng([family number, seed, index]) and nothing else is kept between draws
(the compiled restatements, the fixed list of degenerate BA windows and tracks_pose_ref's memo of restated pairs are
caches of values that depend on nothing else).  The scenes come from the builders the hand-picked tests use, the
expected results from their references: numpy for the matcher (brute force) and the corners (tests/gftt_ref.py,
tests/gftt_topup_ref.py), the sequential restatements under tests/cpp/ for the rest.  run(family, ctx, d) makes the
calls on a context, compare(family, got, d) compares every fetched array bit for bit (floats as bit patterns; where
an entry fetches whole arrays -- the top-up block, the tracks-pose block -- the zero tails past every list too).

Only calls that DESIGN.md §9 and include/orbx.h define are drawn; no draw is one the host layer refuses.

tests/test_side_random_ref.py checks the draws on the CPU (classes covered, restatement against numpy),
tests/test_side_random.py runs them on the GPU, tools/fuzz_sides.py runs an open index range."""
import atexit
import contextlib
import ctypes as C
import importlib
import os
import pathlib
import shutil
import subprocess
import sys
import tempfile

import numpy as np

import carry_ref as CR
import gftt_ref as G
import gftt_topup_ref as T
import landmarks_ref as LR
import landmarks_seq as LS
import landmarks_views_seq as VS
import oracle_lib as O
import pnp_seq as PS
import reassoc_ref as RR
import stitch_seq as SS
import tracks_pose_ref as TR
import window_poses_ref as WR
import window_poses_seq as WS
import test_ba as BA
import test_matcher as M
import test_pose as TP
import test_scale as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuzz_parity  # noqa: E402  (its image kinds)

FAMILIES = ("matcher", "pose", "scale", "ba", "corners", "tracks", "landmarks", "pnp", "carry", "reloc")
# the one small context every draw of a test or a campaign runs on
CONTEXT = dict(max_width=160, max_height=160, max_batch=8)

# ---- the boundary values the issue names (the CPU test asserts that the fixed seeds draw each of them) ---------------
MATCH_SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 513)
MATCH_RATIOS = (0.7, 0.8, 1.0)
POSE_N = (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129)
POSE_ITERS = (0, 1, 31, 32, 33, 64, 65)
POSE_PROB = (0.5, 0.99, 0.999)
POSE_THRESHOLD = (0.5, 1.0, 2.0)
SCALE_N = (0, 1, 2, 255, 256, 257)
BA_LANDMARKS = (1, 7, 63, 256, 257)
BA_SIGMA = (0.0, 0.3)
BA_DELTA = (1.0, 2.5)
LM_SLOTS = (1, 63, 64, 65, 257)
LM_BUILDS = ("plain", "chained", "first_two", "widest", "all_views")
BA_SKIPPED = 3
TRACK_SLOTS = (1, 5, 63, 64, 65, 255, 256, 257)
GF_WIDTHS = (63, 64, 65, 127, 128, 129)
GF_QUALITY = (0.001, 0.01, 0.1, 0.5)
GF_DISTANCES = (0.0, 0.5, 1.0)
GF_MAX_CORNERS = (1, 5, 64, 65, 2000)
GF_SEED_COUNTS = (1, 255, 256, 257)
GF_LDS_KEYS = 8192  # k_gftt_select sorts candidate lists up to this length in LDS, longer ones in the key pool
PNP_SLOTS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 513)
PNP_WINDOW_LEN = (3, 4, 5, 8)
PNP_ITERS = (0, 1, 63, 64, 65, 128, 300)
PNP_PROB = (0.5, 0.99, 0.999)
PNP_THRESHOLD = (0.5, 1.0, 2.0)
PNP_REFINE = (0, 1, 10, 20)
PNP_MIN_INLIERS = (4, 30)
PNP_KINDS = ("clean", "outliers", "ragged", "baseline", "three", "junk", "plane", "padded")
PNP_CHUNK = 64     # k_pnp_ransac solves this many samples per round
PNP_LANES = 256    # ... with a workgroup of this many lanes: every `p += PNP_THREADS` loop runs twice beyond it
CARRY_SLOTS = (1, 5, 63, 64, 65, 255, 256, 257, 513)
CARRY_KINDS = ("generations", "outliers", "origins", "ragged", "old_baseline", "old_bad_pose", "three", "junk")
RELOC_WIDTHS = (41, 42, 43, 63, 64, 65, 66, 67, 127, 128, 129, 157, 158, 159, 160)
RELOC_HEIGHTS = (41, 47, 48, 49, 63, 64, 65, 160)
RELOC_SLOTS = (1, 3, 4, 5, 255, 256, 257, 513)
RA_CAPS = (1, 2, 255, 256, 257, 512, 513)
RA_KINDS = ("flipped", "pool", "mixed", "one", "none")
RA_RATIOS = (0.7, 0.8, 1.0)
RA_MAX_DISTANCE = (0, 40, 256)
RA_INPUTS = ("arrays", "banks", "host")
# the contexts of the reloc family: the level-0 kind (blur_levels 2: the blur of blur_kind; otherwise the copy) and
# patch_size are context parameters.  Draw `index` runs on RELOC_CONTEXTS[(index // 4) % 5]
RELOC_CONTEXTS = (dict(blur_levels=0, blur_kind=0, patch_size=31), dict(blur_levels=2, blur_kind=0, patch_size=9),
                  dict(blur_levels=2, blur_kind=1, patch_size=15), dict(blur_levels=1, blur_kind=0, patch_size=1),
                  dict(blur_levels=2, blur_kind=0, patch_size=41))
RELOC_LEVEL0 = ("copy", "sep16", "k273", "copy", "sep16")  # what RELOC_CONTEXTS[i] describes on

_LIBS = {}
_TMP = []


def seq_lib(name):
    """tests/cpp/<name>_sequential.cpp compiled once per process, with the prototypes the test modules' fixtures set"""
    if name in _LIBS:
        return _LIBS[name]
    if not _TMP:
        _TMP.append(tempfile.mkdtemp(prefix="side_random_"))
        atexit.register(shutil.rmtree, _TMP[0], ignore_errors=True)
    if name == "pnp":  # (its prototypes are pnp_seq's)
        _LIBS[name] = PS.compile_so(pathlib.Path(_TMP[0]))
        return _LIBS[name]
    out = os.path.join(_TMP[0], name + "_sequential.so")  # (pose, scale, ba, st, wp, lm, lm_views)
    subprocess.check_call(TS.CXX + ["-o", out, os.path.join(ROOT, "tests", "cpp", name + "_sequential.cpp")])
    lib = C.CDLL(out)
    DP = C.POINTER(C.c_double)
    if name == "pose":
        lib.seq_solve5.argtypes = [DP, DP]
        lib.seq_estimate_pose.argtypes = [C.c_void_p, C.c_void_p, C.c_int, DP, C.c_double, C.c_double, C.c_int,
                                          C.c_uint64] + [C.c_void_p] * 7
    elif name == "scale":
        lib.seq_triangulate_homogeneous.argtypes = [C.c_void_p, C.c_void_p, C.c_int, DP, DP, DP, C.c_void_p]
        lib.seq_triangulate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, DP, DP, DP, C.c_void_p, C.c_void_p]
        lib.seq_estimate_scale.restype = C.c_double
        lib.seq_estimate_scale.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                           C.POINTER(C.c_int)]
        lib.seq_join_scale.restype = C.c_double
        lib.seq_join_scale.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, DP, DP, C.c_void_p, C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int),
                                       C.POINTER(C.c_int)]
    _LIBS[name] = lib
    return lib


def _rng(family, seed, index):
    return np.random.default_rng([FAMILIES.index(family), int(seed), int(index)])


def _pick(rng, index, salt, values, lo, hi):
    """Every other index (shifted by salt) takes the next boundary value in turn, the rest a uniform integer in
    [lo, hi]: a run of 2 * len(values) consecutive indices holds every boundary value, whatever the seed.  The
    generator is consumed alike on both branches."""
    u = int(rng.integers(lo, hi + 1))
    k = index + salt
    return values[(k // 2) % len(values)] if k % 2 == 0 else u


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- matcher -----------------------------------------------------------------------------------------------------
def np_match_ratio(idx, dist, ratio):
    """`m.distance < ratio * n.distance` on float distances (DMatch::distance), queries with two neighbours only"""
    d = dist.astype(np.float32).astype(np.float64)
    keep = (idx[:, 1] >= 0) & (d[:, 0] < ratio * d[:, 1])
    return np.flatnonzero(keep).astype(np.int32), idx[keep, 0].astype(np.int32), dist[keep, 0].astype(np.int32)


def draw_matcher(seed, index):
    rng = _rng("matcher", seed, index)
    nq = _pick(rng, index, 0, MATCH_SIZES, 0, 600)
    nt = _pick(rng, index, 7, MATCH_SIZES, 0, 600)  # (salt 7: an odd shift, so nq and nt are boundary values in turn)
    if index % 4 == 0:  # both on a boundary (nt would be uniform here)
        nt = MATCH_SIZES[(index // 4) % len(MATCH_SIZES)]
    ratio = MATCH_RATIOS[index % 3]
    kind = ("near", "tie_heavy", "duplicates", "identical")[int(rng.integers(0, 4))]
    s = int(rng.integers(0, 2**31))
    if kind == "near":
        t = M.rand_desc(s, nt)
        q = M.rand_desc(s + 1, nq, near=t, flips=int(rng.choice([1, 2, 6, 20])))
    elif kind == "tie_heavy":
        q, t = M.tie_heavy(nq, nt, seed=s)
    elif kind == "duplicates":  # exact copies inside the train set and of train descriptors among the queries
        t = M.rand_desc(s, nt)
        if nt >= 2:
            src = rng.integers(0, nt, nt // 3 + 1)
            t[rng.integers(0, nt, nt // 3 + 1)] = t[src]
        q = M.rand_desc(s + 1, nq, near=t, flips=3)
        if nq and nt:
            q[rng.integers(0, nq, nq // 4 + 1)] = t[rng.integers(0, nt, nq // 4 + 1)]
    else:
        one = M.rand_desc(s, 1)
        q, t = np.repeat(one, nq, 0), np.repeat(one, nt, 0)
    q, t = np.ascontiguousarray(q).reshape(-1, 32), np.ascontiguousarray(t).reshape(-1, 32)
    idx, dist = M.np_knn2(q, t)
    return dict(family="matcher", seed=seed, index=index, kind=kind, q=q, t=t, ratio=ratio,
                expected=dict(idx=idx, dist=dist, match=np_match_ratio(idx, dist, ratio)))


def run_matcher(c, d):
    idx, dist = c.knn2(d["q"], d["t"])
    return dict(idx=idx, dist=dist, match=c.match_ratio(d["q"], d["t"], d["ratio"]))


def diff_matcher(got, exp):
    out = [k for k in ("idx", "dist") if not same_bits(got[k], exp[k])]
    out += ["match[%d]" % i for i, (a, b) in enumerate(zip(got["match"], exp["match"])) if not same_bits(a, b)]
    return out


# ---- relative pose -----------------------------------------------------------------------------------------------
def draw_pose(seed, index, expected=True):
    rng = _rng("pose", seed, index)
    n = _pick(rng, index, 0, POSE_N, 6, 300)
    max_iters = _pick(rng, index, 3, POSE_ITERS, 2, 200)
    prob = POSE_PROB[int(rng.integers(0, 3))]
    threshold = POSE_THRESHOLD[int(rng.integers(0, 3))]
    K = TP.K_ANISO if rng.random() < 0.4 else TP.K_KITTI
    outliers = float(rng.uniform(0.0, 0.6))
    noise = ("sigma", "round")[int(rng.integers(0, 2))]
    rseed = int(rng.integers(0, 2**32)) if rng.random() < 0.5 else int(rng.integers(2**32, 2**64, dtype=np.uint64))
    variant = ("plain", "plain", "plain", "repeated", "repeated", "equal")[int(rng.integers(0, 6))]
    p1, p2, *_ = TP.scene(int(rng.integers(0, 2**31)), max(n, 1), outliers, noise, K=K)
    p1, p2 = p1[:n].copy(), p2[:n].copy()
    if variant == "repeated" and n >= 2:  # a third of the correspondences are copies of others
        dst, src = rng.integers(0, n, n // 3 + 1), rng.integers(0, n, n // 3 + 1)
        p1[dst], p2[dst] = p1[src], p2[src]
    elif variant == "equal" and n >= 1:
        p1[:], p2[:] = p1[0], p2[0]
    kw = dict(prob=prob, threshold=threshold, max_iters=max_iters, seed=rseed)
    d = dict(family="pose", seed=seed, index=index, variant=variant, outliers=outliers, noise=noise, p1=p1, p2=p2, K=K,
             kw=kw)
    if expected:
        d["expected"] = TP.seq_pose(seq_lib("pose"), p1, p2, K=K, **kw)
    return d


def run_pose(c, d):
    return c.estimate_pose(d["p1"], d["p2"], d["K"], **d["kw"])


def diff_pose(got, exp):
    out = [k for k in ("E", "R", "t", "mask") if not same_bits(got[k], exp[k])]
    return out + [k for k in ("inliers", "good", "iters") if got[k] != exp[k]]


# ---- triangulation and scale -------------------------------------------------------------------------------------
# 3e19 squared is beyond a float: the distance to such a point is +inf, its ratio inf / inf or inf / finite
FAR = np.float32(3e19)


def _flags(rng, n, kind):
    """NULL (0), all-zero (1) or random (2) validity flags"""
    r = (rng.random(n) < 0.8).astype(np.uint8)
    return None if kind == 0 else np.zeros(n, np.uint8) if kind == 1 else r


def draw_scale(seed, index, expected=True):
    """Two triangulations (the pairs of a three-frame scene; now and then under the degenerate pose R = I, t = 0, with
    identical point pairs mixed in) and one scale estimate, either on their points and flags or on hand-made lists."""
    rng = _rng("scale", seed, index)
    n = _pick(rng, index, 0, SCALE_N, 3, 700)
    n_prev = _pick(rng, index, 1, SCALE_N, 3, 700)
    n_cur = _pick(rng, index, 5, SCALE_N, 3, 700)
    noise = ("none", "sigma", "round")[int(rng.integers(0, 3))]
    sc = TS.scene3(int(rng.integers(0, 2**31)), max(n, 1), noise)
    (_, _, a1, a2), (_, _, b2, b3) = sc["pair12"], sc["pair23"]
    a1, a2, b2, b3 = (np.ascontiguousarray(p[:n]) for p in (a1, a2, b2, b3))
    regular = np.ones((2, n), bool)  # correspondences of a sound two-view problem (what numpy's SVD is compared on)
    pose = "degenerate" if rng.random() < 0.2 else "true"
    if pose == "degenerate":
        I, z = np.eye(3), np.zeros(3)
        tri = [(a1, a2, I, z), (b2, b3, I, z)]
        regular[:] = False
    else:
        tri = [(a1, a2, sc["R12"], sc["t12"]), (b2, b3, sc["R23"], sc["t23"])]
    if n and rng.random() < 0.5:  # identical point pairs (parallel rays), one of them the principal point
        a2, b3 = a2.copy(), b3.copy()
        same = rng.integers(0, n, n // 8 + 1)
        a2[same] = a1[same]
        b3[same] = b2[same]
        a1 = a1.copy()
        a1[same[0]] = a2[same[0]] = np.float32([TP.K_KITTI[0, 2], TP.K_KITTI[1, 2]])
        regular[:, same] = False
        tri = [(a1, a2) + tri[0][2:], (b2, b3) + tri[1][2:]]
    d = dict(family="scale", seed=seed, index=index, pose=pose, tri=tri, regular=regular, K=TP.K_KITTI)
    # the kind of the scale call's lists goes by the index, two draws each: one of a pair has boundary lengths
    kind = ("triangulated", "noisy", "lattice", "far")[(index // 2) % 4]
    source = "triangulated" if kind == "triangulated" else "lists"
    lists_rng = np.random.default_rng(int(rng.integers(0, 2**31)))
    d.update(source=source, kind=kind, n_prev=n_prev, n_cur=n_cur, lists_rng=lists_rng)
    if expected:
        finish_scale(d)
    return d


def finish_scale(d):
    """the expected results of a scale draw; the scale call's lists follow from the expected triangulations"""
    lib = seq_lib("scale")
    exp_tri = [TS.seq_triangulate(lib, p, q, R, t, K=d["K"]) for p, q, R, t in d["tri"]]
    rng = d.pop("lists_rng")
    n_prev, n_cur = d["n_prev"], d["n_cur"]
    if d["source"] == "triangulated":  # the two pairs' points, unequal lengths, flags as triangulated / NULL / mixed
        (x12, v12), (x23, v23) = exp_tri
        drop = int(rng.integers(0, 4))
        prev, pv = x12[:max(len(x12) - drop, 0)], v12[:max(len(v12) - drop, 0)]
        cur, cv = x23, v23
        which = int(rng.integers(0, 3))
        pv, cv = (pv, cv) if which == 0 else (None, None) if which == 1 else (pv, None)
    else:
        kind = d["kind"]
        m = max(n_prev, n_cur)
        if kind == "lattice":  # few distinct points: many ratios are the same double, around the median too
            a = rng.integers(-2, 3, (m, 3)).astype(np.float32)
            b = (a * np.float32(0.5))
            b[rng.integers(0, max(m, 1), m // 5)] += np.float32(1.0)
        else:
            a = rng.normal(0, 10, (m, 3)).astype(np.float32)
            b = (a / np.float32(rng.uniform(0.05, 30.0)) + rng.normal(0, 0.05, (m, 3))).astype(np.float32)
            if m:  # repeated points: distances of 0 in either list
                a[rng.integers(0, m, m // 10)] = a[0]
                b[rng.integers(0, m, m // 10)] = b[0]
        both = min(n_prev, n_cur)
        if kind == "far" and both >= 2:  # inside the aligned part: inf / finite, finite / inf and inf / inf
            for arrs in ((a,), (b,), (a, b)):
                i, k = int(rng.integers(0, both)), int(rng.integers(0, 3))
                for arr in arrs:
                    arr[i, k] = FAR
        prev, cur = np.ascontiguousarray(a[:n_prev]), np.ascontiguousarray(b[:n_cur])
        # NULL, all-zero and random flags on either side: the nine combinations in nine consecutive draws
        pv, cv = _flags(rng, n_prev, d["index"] % 3), _flags(rng, n_cur, (d["index"] // 3) % 3)
    d["lists"] = (prev, cur, pv, cv)
    d["expected"] = dict(tri=exp_tri, scale=TS.seq_scale(lib, prev, cur, pv, cv))
    return d


def run_scale(c, d):
    tri = [c.triangulate(p, q, d["K"], R, t) for p, q, R, t in d["tri"]]
    return dict(tri=tri, scale=c.estimate_scale(*d["lists"]))


def diff_scale(got, exp):
    out = []
    for i, ((x, v), (rx, rv)) in enumerate(zip(got["tri"], exp["tri"])):
        out += ["tri[%d].%s" % (i, k) for k, a, b in (("xyz", x, rx), ("valid", v, rv)) if not same_bits(a, b)]
    g, e = got["scale"], exp["scale"]
    if np.float64(g[0]).tobytes() != np.float64(e[0]).tobytes() or g[1] != e[1]:
        out.append("scale %r != %r" % (g, e))
    return out


# ---- bundle adjustment -------------------------------------------------------------------------------------------
_DEGENERATE = []


def _degenerate_windows():
    if not _DEGENERATE:
        _DEGENERATE.extend(BA.degenerate_windows())
    return _DEGENERATE


def _tup(w):
    return (w["poses0"], w["pts0"], w["obs_point"], w["obs_pose"], w["obs_xy"])


def draw_ba(seed, index, expected=True):
    rng = _rng("ba", seed, index)
    nwin = int(rng.integers(1, 13))
    delta = BA_DELTA[int(rng.integers(0, 2))]
    max_iters = int(rng.integers(1, 31))
    windows, names = [], []
    for k in range(nwin):
        W = int(rng.integers(2, 9))
        # (the boundary counts in turn over the windows of consecutive draws; most windows are small, so that a
        # draw of twelve windows stays cheap for the restatement)
        n = _pick(rng, 12 * index + k, 0, BA_LANDMARKS, 2, 300 if rng.random() < 0.25 else 60)
        sigma = BA_SIGMA[int(rng.integers(0, 2))]
        outl = float(rng.choice([0.0, 0.0, 0.05, 0.2]))
        s = int(rng.integers(0, 2**31))
        hard = rng.random() < 0.15  # a start far from the truth: steps get rejected, the iteration limit is met
        if rng.random() < 0.1:
            name, w, _, _ = _degenerate_windows()[int(rng.integers(0, len(_degenerate_windows())))]
        else:
            name = "W%d n%d s%g o%g%s" % (W, n, sigma, outl, " hard" if hard else "")
            w = BA.make_window(s, W, n, sigma=sigma, outliers=outl,
                               **(dict(rot_pert=0.05, t_pert=0.5, x_pert=2.0) if hard else {}))
        windows.append(w)
        names.append(name)
    d = dict(family="ba", seed=seed, index=index, windows=windows, names=names, delta=delta, max_iters=max_iters,
             K=BA.K_KITTI)
    if expected:
        lib = seq_lib("ba")
        d["expected"] = [BA.seq_ba(lib, w, delta=delta, max_iters=max_iters) for w in windows]
    return d


def run_ba(c, d):
    return c.bundle_adjust_batch(d["K"], [_tup(w) for w in d["windows"]], huber_delta=d["delta"],
                                 max_iters=d["max_iters"])


def diff_ba(got, exp):
    if len(got) != len(exp):
        return ["%d windows != %d" % (len(got), len(exp))]
    return ["window %d: %r != %r" % (k, g[2], e[2]) for k, (g, e) in enumerate(zip(got, exp)) if not BA.same(g, e)]


# ---- Shi-Tomasi corners: batch, top-up, mask entry ---------------------------------------------------------------
def blocks_image(h, w):
    """2 x 2 blocks in a checkerboard: by its symmetries every interior pixel has the same response, so every one of
    them is a candidate -- the only frame of 160 x 160 or less whose candidate list outgrows GF_LDS_KEYS"""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((yy // 2) + (xx // 2)) % 2 == 0, 20, 220).astype(np.uint8)


def _seeds(rng, corners, cap, h, w):
    """cap seed slots: near detected corners, anywhere in the frame, on the last row or column, and slots rule A
    drops (NaN, infinite, just outside)"""
    out = np.empty((cap, 2), np.float32)
    inf = np.float32("inf")
    for s in range(cap):
        k = int(rng.integers(0, 10))
        if k < 4 and len(corners):
            out[s] = corners[int(rng.integers(0, len(corners)))] + rng.uniform(-0.49, 0.49, 2)
        elif k < 6:
            out[s] = (rng.uniform(0, w - 1), rng.uniform(0, h - 1))
        elif k == 6:
            out[s] = [(w - 1, rng.uniform(0, h - 1)), (rng.uniform(0, w - 1), h - 1), (w - 1, h - 1), (0, 0)][int(rng.integers(0, 4))]
        elif k == 7:
            out[s] = [(np.nan, 5), (5, np.nan), (inf, 5), (5, -inf)][int(rng.integers(0, 4))]
        elif k == 8:
            out[s] = [(-0.001, 5), (w - 1 + 0.001, 5), (5, -0.001), (5, h - 1 + 0.001), (-40, 3), (3, h + 40)][int(rng.integers(0, 6))]
        else:
            out[s] = (float(rng.integers(0, w)), float(rng.integers(0, h)))  # on a pixel: distance ties at d
    return out


def draw_corners(seed, index):
    rng = _rng("corners", seed, index)
    w = _pick(rng, index, 0, GF_WIDTHS, 8, 160)
    h = int(rng.integers(8, 161))
    if index % 16 == 7:  # the smallest frames in turn, and the largest
        h = 8 + (index // 16) % 5
    elif index % 16 == 15:
        h = 160 - (index // 16) % 3
    nf = int(rng.integers(1, 7))
    quality = GF_QUALITY[int(rng.integers(0, 4))]
    u = float(rng.uniform(1.0, 12.0))
    dist = GF_DISTANCES[(index // 2) % 3] if index % 2 else u
    max_corners = (GF_MAX_CORNERS + (2000, 2000))[int(rng.integers(0, 7))]  # (small caps fill with carried seeds)
    masked_max = ((0,) + GF_MAX_CORNERS)[int(rng.integers(0, 6))]  # 0: no limit (the host entries only)
    blocks = index % 8 == 5
    if blocks:  # (the candidate list beyond the LDS sort needs more than GF_LDS_KEYS interior pixels)
        h, w, nf = max(h, 100), max(w, 100), min(nf, 3)
    frames = np.stack([fuzz_parity.image(rng, h, w) for _ in range(nf)])
    if blocks:
        frames[int(rng.integers(0, nf))] = blocks_image(h, w)
        if rng.random() < 0.5:
            quality, dist = 0.01, float(rng.choice([0.0, 1.0, 3.0]))
    # frames as regions of a parent buffer: odd base, row stride and gaps, garbage around them
    strided = rng.random() < 0.4
    base, rs = int(rng.integers(0, 8)), w + int(rng.integers(0, 20))
    fs = rs * h + int(rng.integers(0, 50))
    garbage = rng.integers(0, 256, base + nf * fs, dtype=np.uint8)
    cap = _pick(rng, index, 1, GF_SEED_COUNTS, 1, 300)
    seeds = np.empty((nf, cap, 2), np.float32)
    plain = [G.good_features_to_track(f, max_corners, quality, dist) for f in frames]
    for f in range(nf):
        seeds[f] = _seeds(rng, plain[f], cap, h, w)
    seen_min = int(rng.integers(0, 4))
    seen = rng.integers(0, 5, (nf, cap)).astype(np.int32) if seen_min else None
    mkind = ("random", "empty", "full", "random")[int(rng.integers(0, 4))]
    mask = {"random": (rng.random((h, w)) < rng.uniform(0.1, 0.95)).astype(np.uint8) * int(rng.integers(1, 256)),
            "empty": np.zeros((h, w), np.uint8), "full": np.full((h, w), 255, np.uint8)}[mkind]
    top = [T.top_up(frames[f], seeds[f], max_corners, quality, dist, seen=None if seen is None else seen[f],
                    seen_min=seen_min, full=True) for f in range(nf)]
    masked, info = T.good_features_to_track_masked(frames[0], mask, masked_max, quality, dist, full=True)
    return dict(family="corners", seed=seed, index=index, frames=frames, strided=strided, layout=(base, rs, fs),
                garbage=garbage, quality=quality, dist=dist, max_corners=max_corners, masked_max=masked_max,
                seeds=seeds, seen=seen, seen_min=seen_min, mask=mask, mask_kind=mkind, blocks=blocks,
                info=dict(top=[t[3] for t in top], masked=info),
                expected=dict(plain=plain, top=T.batch_arrays(top, max_corners), masked=masked))


def run_corners(c, d):
    import torch

    frames = d["frames"]
    nf, h, w = frames.shape
    if d["strided"]:
        base, rs, fs = d["layout"]
        buf = d["garbage"].copy()
        np.lib.stride_tricks.as_strided(buf[base:], shape=(nf, h, w), strides=(fs, rs, 1))[...] = frames
        t = torch.as_strided(torch.from_numpy(buf).cuda(), (nf, h, w), (fs, rs, 1), base)
    else:
        t = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    params = (d["max_corners"], d["quality"], d["dist"])
    c.good_features_batch(t, *params)
    plain = c.good_features_fetch()
    c.good_features_topup(t, d["seeds"], d["seen"], d["seen_min"], max_corners=params[0], quality_level=params[1],
                          min_distance=params[2])
    top = c.good_features_topup_fetch()
    masked = c.good_features_to_track_masked(frames[0], d["mask"], d["masked_max"], d["quality"], d["dist"])
    return dict(plain=plain, top=top, masked=masked)


def diff_corners(got, exp):
    out = []
    if len(got["plain"]) != len(exp["plain"]):
        out.append("plain: %d frames != %d" % (len(got["plain"]), len(exp["plain"])))
    out += ["plain[%d]" % f for f, (a, b) in enumerate(zip(got["plain"], exp["plain"])) if not same_bits(a, b)]
    out += ["top.%s" % k for k, a, b in zip(("counts", "carried", "points", "origin"), got["top"], exp["top"])
            if not same_bits(a, b)]  # whole arrays: zero / -1 at and beyond counts[f]
    if not same_bits(got["masked"], exp["masked"]):
        out.append("masked")
    return out


# ---- tracks pose -> the stream's chain -> stitch -----------------------------------------------------------------
def _start_pose(rng):
    return WR.rigid(WR.rot(rng.normal(size=3), 0.8), rng.normal(size=3) * 4.0)


def draw_tracks(seed, index):
    """Windows of tracked slots (tracks_pose_ref.window, a pattern per window) through orbx_tracks_pose_device, then
    orbx_window_poses_stream_device on that block, then orbx_stitch_windows_device on the chain's block."""
    rng = _rng("tracks", seed, index)
    cap = _pick(rng, index, 0, TRACK_SLOTS, 2, 300)
    L = int(rng.integers(2, 7))
    n = int(rng.integers(1, 8))
    if cap > 128:  # (the large blocks with fewer windows: the restatement's time goes with slots x pairs)
        n = min(n, 3)
    patterns = tuple(TR.PATTERNS[int(rng.integers(0, len(TR.PATTERNS)))] for _ in range(n))
    K = TP.K_ANISO if rng.random() < 0.4 else TP.K_KITTI
    stride = int(rng.integers(1, L))
    align = bool(stride <= L - 2 and rng.random() < 0.6)
    T_start = _start_pose(rng) if rng.random() < 0.5 else None
    first = float(rng.choice([1.0, 0.5 + stride, 0.1, 5.0]))
    kw = dict(prob=POSE_PROB[int(rng.integers(0, 3))], threshold=POSE_THRESHOLD[int(rng.integers(0, 3))],
              max_iters=_pick(rng, index, 1, POSE_ITERS, 2, 100),
              seed=int(rng.integers(0, 2**32)) if rng.random() < 0.5 else int(rng.integers(2**32, 2**64, dtype=np.uint64)))
    ws = [TR.window(int(rng.integers(0, 2**31)), cap, L, p, K) for p in patterns]
    tracks, seen = np.stack([w[0] for w in ws]), np.stack([w[1] for w in ws])
    pairs = TR.restate((seq_lib("pose"), seq_lib("scale")), K, tracks, seen, **kw)
    tp = TR.block(pairs, cap)
    scale = tp["scale"].reshape(n, L - 1)
    s0 = SS.seq_scale0(seq_lib("st"), scale, stride, first)
    wp = WS.seq_chain(seq_lib("wp"), None, s0, tp["R"].reshape(n, L - 1, 3, 3), tp["t"].reshape(n, L - 1, 3), scale)
    st = SS.seq_stitch(seq_lib("st"), wp["poses4x4"], stride, T_start, align)
    return dict(family="tracks", seed=seed, index=index, cap=cap, L=L, patterns=patterns, K=K, stride=stride,
                align=align, T_start=T_start, first=first, kw=kw, tracks=tracks, seen=seen, pairs=pairs, s0=s0,
                expected=dict(tp=tp, wp=wp, st=st))


def run_tracks(c, d):
    import torch

    pkg = importlib.import_module("visual-odometry-gpu_amd")
    t, s = torch.from_numpy(d["tracks"]).cuda(), torch.from_numpy(d["seen"]).cuda()
    torch.cuda.synchronize()
    c.tracks_pose(d["K"], t, s, **d["kw"])
    f = c.tracks_pose_fetch()  # waits for the call
    v = c.tracks_pose_view()
    m, cap = v.n_pairs, v.slot_capacity
    tp = dict(f, E=f["E"].reshape(m, 9), R=f["R"].reshape(m, 9), slot_of=np.zeros((m, cap), np.int32),
              mask=np.zeros((m, cap), np.uint8), xyz=np.zeros((m, cap, 3), np.float32),
              valid=np.zeros((m, cap), np.uint8))
    hip = pkg.orbx.load()
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    for k in ("slot_of", "mask", "xyz", "valid"):  # every row to its full slot capacity: the zero tails too
        if hip.hipMemcpy(tp[k].ctypes.data, getattr(v, k), tp[k].nbytes, 2) != 0:
            raise RuntimeError("hipMemcpy of the tracks-pose block failed")
    pkg.orbx_stream.window_poses_stream(c, d["stride"], d["first"])
    wp = pkg.orbx_vo.window_poses_fetch(c)
    pkg.orbx_stream.stitch_windows_device(c, pkg.orbx_vo.window_poses_view(c), d["stride"], d["T_start"], d["align"])
    return dict(tp=tp, wp=wp, st=pkg.orbx_stream.stitch_fetch(c))


def diff_tracks(got, exp):
    out = []
    for part in ("tp", "wp", "st"):
        if set(got[part]) != set(exp[part]):
            out.append("%s: keys %s != %s" % (part, sorted(got[part]), sorted(exp[part])))
            continue
        out += ["%s.%s" % (part, k) for k in exp[part] if not SS.bits_equal(got[part][k], exp[part][k])]
    return out


# ---- landmarks -> solve -> write-back ----------------------------------------------------------------------------
LM_SCENES = ("noisy", "tilted", "behind", "baseline", "bad_pose", "nan_observation", "ragged", "clean")


def _lm_scene(rng, kind, W, slots, min_seen, gated):
    s = int(rng.integers(0, 2**31))
    if kind == "noisy":
        sc = LR.make_scene(s, W=W, slots=slots, min_seen=min_seen, sigma=0.3, outliers=0.1, pose_pert=0.002)
    elif kind == "tilted":
        sc = LR.make_scene(s, W=W, slots=slots, min_seen=min_seen, world=LR.WORLD_TILTED, sigma=0.3, outliers=0.1,
                           pose_pert=0.002)
    elif kind == "behind":
        sc = LR.make_scene(s, W=W, slots=slots, min_seen=min_seen, depth_sign=-1.0)
    elif kind == "baseline":
        sc = LR.make_scene(s, W=W, slots=slots, min_seen=min_seen, step=0.05)
    elif kind == "ragged":
        sc = LR.make_scene(s, W=W, slots=slots, min_seen=0, sigma=0.3, outliers=0.3)
    else:
        sc = LR.make_scene(s, W=W, slots=slots, min_seen=min_seen, pose_pert=0.002 if kind == "clean" else 0.0)
    if kind == "bad_pose":  # a rotation angle beyond 1e5 rad: one of the first two poses, or a later one
        sc["poses"][int(rng.integers(0, W)), :3] = np.array([0.0, 2e5, 0.0])
    if kind == "nan_observation":
        # One observed pixel is not finite -- in a view that keeps the landmark out of the block: any observed view
        # when there is a gate (reproj_px is +inf there: ORBX_LM_REPROJECTION), view 0 without one (view 0 is among
        # the triangulating views of every mode: "h[3] == 0 or a quotient that is not finite: ORBX_LM_DEGENERATE").
        # A landmark that reached the solve with such a pixel would end it as ORBX_BA_FAILURE ("non-finite initial
        # cost"), and the rules say no more about that summary: its costs are NaN, and IEEE 754 leaves the sign and
        # payload of an invalid operation's NaN to the implementation (negative on x86, positive on the GPU).
        live = np.flatnonzero(sc["seen"] >= 1)
        if len(live):
            slot = sc["bad_slot"] = int(live[int(rng.integers(0, len(live)))])
            view = int(rng.integers(0, sc["seen"][slot])) if gated else 0
            sc["tracks"][slot, view, int(rng.integers(0, 2))] = np.float32([np.nan, np.inf][int(rng.integers(0, 2))])
    return sc


def draw_landmarks(seed, index):
    """A batch of windows through one of the five builds (orbx_landmarks_build_device on host poses, the chained build
    behind tracks pose and the window-pose chain, and the views build in its three modes with a gate of 0 or 3 px),
    then orbx_bundle_adjust_landmarks_device and orbx_bundle_adjust_write_back_device."""
    rng = _rng("landmarks", seed, index)
    slots = _pick(rng, index, 0, LM_SLOTS, 2, 300)
    W = int(rng.integers(2, 9))
    n = int(rng.integers(1, 7))
    if slots > 128:  # (the restated solve's time goes with slots x windows)
        n = min(n, 3)
    build = LM_BUILDS[index % 5]
    gate = (0.0, 3.0)[(index // 5) % 2]
    min_seen = (0, W)[int(rng.integers(0, 2))]
    kinds = tuple(LM_SCENES[int(rng.integers(0, len(LM_SCENES)))] for _ in range(n))
    scenes = [_lm_scene(rng, k, W, slots, min_seen, build in LM_BUILDS[2:] and gate > 0) for k in kinds]
    poses, tracks, seen = LR.stack(scenes)
    delta = BA_DELTA[int(rng.integers(0, 2))]
    max_iters = int(rng.integers(1, 21))
    K = LR.K_KITTI
    d = dict(family="landmarks", seed=seed, index=index, slots=slots, W=W, build=build, gate=gate, kinds=kinds,
             min_seen=min_seen, scenes=scenes, tracks=tracks, seen=seen, K=K, delta=delta, max_iters=max_iters)
    exp = {}
    if build == "chained":  # the poses come from the tracks themselves, on the device
        kw = dict(prob=0.999, threshold=1.0, max_iters=int(rng.integers(0, 101)), seed=int(rng.integers(0, 2**32)))
        tp = TR.block(TR.restate((seq_lib("pose"), seq_lib("scale")), K, tracks, seen, **kw), slots)
        wp = WS.seq_chain(seq_lib("wp"), None, None, tp["R"].reshape(n, W - 1, 3, 3), tp["t"].reshape(n, W - 1, 3),
                          tp["scale"].reshape(n, W - 1))
        assert (wp["status"] == WR.OK).all()  # (a chain of a tracks block is finite)
        poses = wp["poses6"]
        d["pose_kw"] = kw
    if build in ("plain", "chained"):
        block = LS.seq_build(seq_lib("lm"), K, poses, tracks, seen)
    else:
        block, exp["reason"], exp["reproj_px"] = VS.seq_views_build(seq_lib("lm_views"), K, poses, tracks, seen,
                                                                    LM_BUILDS.index(build) - 2, gate)
    solved, sums, pts = np.array(poses, np.float64), [], []
    for w in range(n):
        if block["status"][w] != LR.OK:
            sums.append(dict(termination=BA_SKIPPED, iterations=0, successful_steps=0, initial_cost=0.0, final_cost=0.0))
            continue
        p3, _, op, oq, xy = LS.window_of(block, w)
        solved[w], x, sm = LS.seq_ba(seq_lib("ba"), K, poses[w], p3, op, oq, xy, delta, max_iters)
        sums.append(sm)
        pts.append(x)
    term = np.array([sm["termination"] for sm in sums], np.int32)
    p4, upd, angle, dist = WS.seq_gate(seq_lib("wp"), solved, poses, term, WR.MAX_ROT_DIFF, WR.MAX_TRANS_DIFF)
    exp.update(block=block, solved=solved, summaries=sums, points=np.concatenate(pts) if pts else np.zeros((0, 3)),
               poses4x4=p4, updated=upd)
    d.update(poses=poses, expected=exp, gate_values=(angle, dist))
    return d


def run_landmarks(c, d):
    import torch

    pkg = importlib.import_module("visual-odometry-gpu_amd")
    LM, VO = pkg.orbx_lm, pkg.orbx_vo
    t, s = torch.from_numpy(d["tracks"]).cuda(), torch.from_numpy(d["seen"]).cuda()
    torch.cuda.synchronize()
    build, got = d["build"], {}
    if build == "plain":
        c.landmarks_build(d["K"], t, s, d["poses"])
    elif build == "chained":
        c.tracks_pose(d["K"], t, s, **d["pose_kw"])
        VO.window_poses(c)
        VO.landmarks_build_chained(c, d["K"], t, s)
    else:
        LM.landmarks_build_views(c, d["K"], t, s, d["poses"], LM_BUILDS.index(build) - 2, d["gate"])
        got["reason"], got["reproj_px"] = LM.landmarks_views_fetch(c)
    got["block"] = c.landmarks_fetch()
    c.bundle_adjust_landmarks(d["delta"], d["max_iters"])
    got["solved"], got["summaries"], got["points"] = c.bundle_adjust_landmarks_fetch()
    VO.bundle_adjust_write_back(c)
    got["poses4x4"], got["updated"] = VO.bundle_adjust_write_back_fetch(c)
    return got


def diff_landmarks(got, exp):
    out = []
    if set(got) != set(exp):
        return ["keys %s != %s" % (sorted(got), sorted(exp))]
    out += ["block.%s" % k for k in LS.KEYS + ("pose_offset",) if not SS.bits_equal(got["block"][k], exp["block"][k])]
    out += [k for k in exp if k not in ("block", "summaries") and not SS.bits_equal(got[k], exp[k])]
    if len(got["summaries"]) != len(exp["summaries"]):
        out.append("summaries: %d != %d" % (len(got["summaries"]), len(exp["summaries"])))
    for w, (g, e) in enumerate(zip(got["summaries"], exp["summaries"])):
        if set(g) != set(e) or any(np.float64(g[k]).tobytes() != np.float64(e[k]).tobytes() for k in e):
            out.append("summary %d: %r != %r" % (w, g, e))
    return out


# ---- window PnP over the landmarks block (rank 17) ---------------------------------------------------------------
def _weighted(rng, names, weights):
    return names[int(rng.choice(len(names), p=np.asarray(weights, float) / sum(weights)))]


def _pnp_params(rng, index):
    """the parameters of a PnP call: max_iters in turn by the index, the others drawn"""
    seed = int(rng.integers(0, 2**32)) if rng.random() < 0.5 else int(rng.integers(2**32, 2**64, dtype=np.uint64))
    return dict(prob=PNP_PROB[int(rng.integers(0, 3))], threshold_px=PNP_THRESHOLD[int(rng.integers(0, 3))],
                max_iters=PNP_ITERS[index % len(PNP_ITERS)], seed=seed,
                refine_iters=PNP_REFINE[int(rng.integers(0, 4))],
                min_inliers=PNP_MIN_INLIERS[int(rng.integers(0, 4)) == 0])


def _pnp_scene(rng, kind, W, cap):
    """One window of `cap` slots by the kinds of test_pnp.batch_scenes: (scene, declared outlier share, live slots)."""
    import test_pnp as TPN

    s = int(rng.integers(0, 2**31))
    share = 0.0
    if kind == "plane" and cap < 4:
        kind = "clean"
    if kind == "outliers":  # 10 to 50 % of the observations of frames >= 2; above 30 % with pixel noise as well
        share = float(rng.uniform(0.1, 0.5))
        sc = LR.make_scene(s, W=W, slots=cap, min_seen=W, outliers=share, pose_pert=0.002,
                           sigma=0.3 if share > 0.3 and rng.random() < 0.5 else 0.0)
        if rng.random() < 0.4:  # one frame with 55 to 75 % of random pixels: RANSAC runs beyond its first chunk there
            k, share = int(rng.integers(2, W)), float(rng.uniform(0.55, 0.75))
            bad = rng.random(cap) < share
            junk = np.c_[rng.uniform(0, LR.IMG_W, cap), rng.uniform(0, LR.IMG_H, cap)].astype(np.float32)
            sc["tracks"][:, k] = np.where((bad & (sc["seen"] > k))[:, None], junk, sc["tracks"][:, k])
    elif kind == "ragged":
        sc = LR.make_scene(s, W=W, slots=cap, min_seen=(0, 2)[int(rng.integers(0, 2))], pose_pert=0.002)
    elif kind == "junk":  # a dozen live slots, one frame >= 2 of random pixels
        live = min(cap, 12)
        sc = TPN.pad(LR.make_scene(s, W=W, slots=live, min_seen=W), cap)
        k = int(rng.integers(2, W))
        sc["tracks"][:live, k] = np.c_[rng.uniform(0, LR.IMG_W, live), rng.uniform(0, LR.IMG_H, live)]
    elif kind == "plane":  # four points of the plane z = 12
        sc = TPN.pad(LR.make_scene(s, W=W, slots=4, min_seen=W), cap)
        pix = np.array([[300.0, 80.0, 1.0], [900.0, 100.0, 1.0], [350.0, 300.0, 1.0], [880.0, 290.0, 1.0]])
        sc["tracks"][:4] = TPN.project(sc["true_poses"], (np.linalg.inv(LR.K_KITTI) @ pix.T).T * 12.0)
    elif kind == "padded":  # seen = 0 behind the live slots: n_corr < cap
        live = int(rng.integers(cap // 2 + 1, cap + 1))
        sc = TPN.pad(LR.make_scene(s, W=W, slots=live, min_seen=W, pose_pert=0.002), cap)
    else:
        sc = LR.make_scene(s, W=W, slots=cap, min_seen=W, pose_pert=0.0 if kind == "baseline" else 0.002)
    if kind == "baseline":
        sc["poses"][1, 3:] = sc["poses"][0, 3:] + np.array([0.01, 0.0, 0.02])
    if kind == "three":
        sc["seen"][3:] = 0
        sc["tracks"][3:] = 0
    return sc, share, int((sc["seen"] >= 2).sum())


def draw_pnp(seed, index):
    """A batch of windows through orbx_landmarks_build_device and orbx_window_poses_pnp_device; on two draws of four
    one of its problems through the host entry orbx_pnp_ransac too, on every fourth one of at most 257 slots the solve
    seeded with the PnP poses (orbx_bundle_adjust_landmarks_pnp_device)."""
    rng = _rng("pnp", seed, index)
    cap = _pick(rng, index, 0, PNP_SLOTS, 1, 600)
    W = PNP_WINDOW_LEN[(index // 2) % 4]
    n = int(rng.integers(1, 7))
    kinds = tuple(_weighted(rng, PNP_KINDS, (3, 3, 1, 1, 1, 1, 1, 2)) for _ in range(n))
    made = [_pnp_scene(rng, k, W, cap) for k in kinds]
    scenes = [m[0] for m in made]
    poses, tracks, seen = LR.stack(scenes)
    params = _pnp_params(rng, index)
    K = LR.K_KITTI
    pnp = seq_lib("pnp")
    block = LS.seq_build(seq_lib("lm"), K, poses, tracks, seen)
    exp = dict(block=block, pnp=PS.windows(pnp, K, block, poses, cap, **params))
    d = dict(family="pnp", seed=seed, index=index, cap=cap, W=W, kinds=kinds, scenes=scenes, params=params, K=K,
             shares=[m[1] for m in made], live=[m[2] for m in made], poses=poses, tracks=tracks, seen=seen,
             host=None, solve=None)
    w, k = int(rng.integers(0, n)), int(rng.integers(2, W))
    delta, ba_iters = BA_DELTA[int(rng.integers(0, 2))], int(rng.integers(1, 21))
    # problem (w, k) on host arrays, under the seed the batch gives frame k: on two draws of four, an odd and an even
    # index, so that the host entry meets the boundary capacities (even indices) and the uniform ones (odd) alike
    if index % 4 in (1, 2):
        pts, _, op, oq, xy = LS.window_of(block, w)
        sel = oq == k
        one = dict(params, seed=int(pnp.seq_pnp_problem_seed(params["seed"], k)))
        d["host"] = dict(w=w, k=k, points3=pts[op[sel]], pixels=xy[sel], params=one)
        exp["host"] = PS.problem(pnp, K, pts[op[sel]], xy[sel], **one)
    if index % 4 == 2 and cap <= 257:  # the solve from the seeded poses, as draw_landmarks restates it
        d["solve"] = dict(delta=delta, max_iters=ba_iters)
        solved, sums, pts3 = np.array(exp["pnp"]["poses6"], np.float64), [], []
        for v in range(n):
            if block["status"][v] != LR.OK:
                sums.append(dict(termination=BA_SKIPPED, iterations=0, successful_steps=0, initial_cost=0.0,
                                 final_cost=0.0))
                continue
            p3, _, op, oq, xy = LS.window_of(block, v)
            solved[v], x, sm = LS.seq_ba(seq_lib("ba"), K, exp["pnp"]["poses6"][v], p3, op, oq, xy, delta, ba_iters)
            sums.append(sm)
            pts3.append(x)
        exp["solve"] = dict(solved=solved, summaries=sums, points=np.concatenate(pts3) if pts3 else np.zeros((0, 3)))
    d["expected"] = exp
    return d


def _fetch_bytes(pkg, address, shape, dtype):
    """a whole device array, its tails included"""
    out = np.zeros(shape, dtype)
    hip = pkg.orbx.load()
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    if out.nbytes and hip.hipMemcpy(out.ctypes.data, address, out.nbytes, 2) != 0:
        raise RuntimeError("hipMemcpy of a result block failed")
    return out


def run_pnp(c, d):
    pkg = importlib.import_module("visual-odometry-gpu_amd")
    PNP = pkg.orbx_pnp
    c.landmarks_build(d["K"], d["tracks"], d["seen"], d["poses"])
    got = dict(block=c.landmarks_fetch())
    PNP.window_poses_pnp(c, **d["params"])
    f = PNP.window_poses_pnp_fetch(c)  # waits for the call
    v = PNP.window_poses_pnp_view(c)
    # every mask row to the slot capacity: the zeros behind a window's points too
    mask = _fetch_bytes(pkg, v.mask, (v.n_windows, v.window_len - 2, v.slot_capacity), np.uint8)
    got["pnp"] = dict(records=f["records"], poses6=f["poses6"], mask=mask)
    got["mask_lists"] = f["masks"]
    if d["host"] is not None:
        h = d["host"]
        got["host"] = PNP.pnp_ransac(c, h["points3"], h["pixels"], d["K"], **h["params"])
        again = PNP.window_poses_pnp_fetch(c, masks=False)  # the batched block is still there behind the host entry
        got["pnp_again"] = dict(records=again["records"], poses6=again["poses6"])
    if d["solve"] is not None:
        PNP.bundle_adjust_landmarks_pnp(c, d["solve"]["delta"], d["solve"]["max_iters"])
        s = c.bundle_adjust_landmarks_fetch()
        got["solve"] = dict(solved=s[0], summaries=s[1], points=s[2])
    return got


def _diff_records(got, exp, name):
    if got.dtype != PS.RECORD or got.shape != exp.shape:
        return ["%s: %s %s != %s" % (name, got.dtype, got.shape, exp.shape)]
    out = ["%s.%s" % (name, k) for k in PS.RECORD.names
           if np.ascontiguousarray(got[k]).tobytes() != np.ascontiguousarray(exp[k]).tobytes()]
    return out or (["%s (padding)" % name] if got.tobytes() != exp.tobytes() else [])


def _diff_summaries(got, exp):
    out = []
    if len(got) != len(exp):
        out.append("summaries: %d != %d" % (len(got), len(exp)))
    for w, (g, e) in enumerate(zip(got, exp)):
        if set(g) != set(e) or any(np.float64(g[k]).tobytes() != np.float64(e[k]).tobytes() for k in e):
            out.append("summary %d: %r != %r" % (w, g, e))
    return out


def diff_pnp(got, exp):
    if "pnp" in got and "mask_lists" not in got:  # an expected result compared with itself (the reproducibility test)
        got = dict(got, mask_lists=None)
    out = ["block.%s" % k for k in LS.KEYS + ("pose_offset",) if not SS.bits_equal(got["block"][k], exp["block"][k])]
    out += _diff_records(got["pnp"]["records"], exp["pnp"]["records"], "records")
    out += ["pnp.%s" % k for k in ("poses6", "mask") if not same_bits(got["pnp"][k], exp["pnp"][k])]
    if got["mask_lists"] is not None:  # what the mask fetch hands out: one byte per point of the window
        off = exp["block"]["point_offset"]
        for w, rows in enumerate(got["mask_lists"]):
            for k, m in enumerate(rows):
                if not same_bits(m, exp["pnp"]["mask"][w, k, :off[w + 1] - off[w]]):
                    out.append("mask fetch (%d, %d)" % (w, k + 2))
    if ("host" in exp) != ("host" in got) or ("solve" in exp) != ("solve" in got):
        return out + ["keys %s != %s" % (sorted(got), sorted(exp))]
    if "host" in exp:
        g, e = got["host"], exp["host"]
        out += ["host.%s" % k for k in ("pose6", "mask") if not same_bits(g[k], e[k])]
        out += ["host.%s" % k for k in ("inliers", "iters", "status") if g[k] != e[k]]
        if np.float64(g["rms_px"]).tobytes() != np.float64(e["rms_px"]).tobytes():
            out.append("host.rms_px")
        if "pnp_again" in got:
            out += _diff_records(got["pnp_again"]["records"], exp["pnp"]["records"], "records behind the host entry")
            if not same_bits(got["pnp_again"]["poses6"], exp["pnp"]["poses6"]):
                out.append("poses6 behind the host entry")
    if "solve" in exp:
        out += ["solve.%s" % k for k in ("solved", "points") if not SS.bits_equal(got["solve"][k], exp["solve"][k])]
        out += _diff_summaries(got["solve"]["summaries"], exp["solve"]["summaries"])
    return out


# ---- landmark carry and the carried PnP (rank 18) ----------------------------------------------------------------
def _carry_window(rng, kind, W, old_cap, cap):
    """One old window of old_cap slots and its successor of cap slots: (old, new), each a dict of tracks and seen (old:
    poses too; new: origin and the share of replaced pixels)."""
    s = int(rng.integers(0, 2**31))
    m = min(old_cap, cap)
    if kind in ("origins", "ragged"):
        # an old window whose seen runs from 0 to W (slots below 2 own no landmark) and a successor put together slot
        # by slot
        live = int(rng.integers(max(1, old_cap // 2), old_cap + 1))
        stream = CR.make_stream(s, 2 * W - 1, live + cap)
        old = CR.window(stream, 0, W, np.arange(live), rng.integers(0, W + 1, live))
        origin, ids = np.full(cap, -1, np.int32), live + np.arange(cap)  # fresh points unless carried
        for t in range(cap):
            u = int(rng.integers(0, 12)) if kind == "origins" else int(rng.integers(0, 4))
            if u < 5:  # an old slot, with or without a landmark
                origin[t] = int(rng.integers(0, live))
                ids[t] = origin[t]
            elif u == 5:  # at or beyond the old capacity
                origin[t] = (old_cap, old_cap + 5, 2**31 - 1)[int(rng.integers(0, 3))]
            elif u == 6:  # negative, other than -1
                origin[t] = (-7, -2, -2**31)[int(rng.integers(0, 3))]
            elif u == 7 and t > 0:  # the origin of the slot before: two new slots name one old slot
                origin[t], ids[t] = origin[t - 1], ids[t - 1]
            elif u == 8:  # a padding slot of the old window
                origin[t] = int(rng.integers(live, old_cap)) if live < old_cap else -1
        seen = np.full(cap, W, np.int32)
        if kind == "ragged":  # 0 .. W + 2, and pixels that are not finite
            seen = rng.integers(0, W + 3, cap).astype(np.int32)
        new = CR.window(stream, W - 1, W, ids, seen)
        new["origin"] = origin
        if kind == "ragged":
            for t in rng.integers(0, cap, cap // 8 + 1):
                new["tracks"][t, int(rng.integers(0, W)), int(rng.integers(0, 2))] = \
                    np.float32([np.nan, np.inf, -np.inf][int(rng.integers(0, 3))])
    else:
        old_slots = m if kind != "junk" else min(m, 12)
        fresh = min(10, cap - old_slots)
        min_seen = W if kind in ("outliers", "junk") or rng.random() < 0.5 else 2
        stream, old, new = CR.two_generations(s % 2**30, W, old_slots, fresh, min_seen=min_seen, cap=cap)
    pad = old_cap - len(old["seen"])
    old = dict(tracks=np.concatenate([old["tracks"], np.zeros((pad, W, 2), np.float32)]),
               seen=np.concatenate([old["seen"], np.zeros(pad, np.int32)]), poses=old["true_poses"].copy(),
               ids=old["ids"])
    share = 0.0
    if kind == "outliers":  # 10 to 50 % of the new window's pixels replaced, in four windows of ten 55 to 75 %
        share = float(rng.uniform(0.1, 0.5)) if rng.random() < 0.6 else float(rng.uniform(0.55, 0.75))
        bad = rng.random((cap, W)) < share
        junk = np.stack([rng.uniform(0, LR.IMG_W, (cap, W)), rng.uniform(0, LR.IMG_H, (cap, W))], -1).astype(np.float32)
        new["tracks"] = np.where(bad[..., None], junk, new["tracks"])
    elif kind == "old_baseline":
        old["poses"][1, 3:] = old["poses"][0, 3:] + np.array([0.01, 0.0, 0.02])
    elif kind == "old_bad_pose":
        old["poses"][int(rng.integers(0, 2)), :3] = np.array([0.0, 2e5, 0.0])
    elif kind == "three":
        new["origin"][3:] = -1
    elif kind == "junk":  # one frame of random pixels: frame 0 or 1 loses the window, a later one keeps the pose before
        k = int(rng.integers(0, W))
        new["tracks"][:, k] = np.c_[rng.uniform(0, LR.IMG_W, cap), rng.uniform(0, LR.IMG_H, cap)]
    new["share"] = share
    return old, new


def draw_carry(seed, index):
    """Old windows through orbx_landmarks_build_device, their successors' origin through orbx_landmarks_carry_device,
    the successors' tracks through orbx_window_poses_pnp_carried_device; the blocks of both fetched whole."""
    rng = _rng("carry", seed, index)
    cap = _pick(rng, index, 0, CARRY_SLOTS, 1, 600)
    old_cap = _pick(rng, index, 5, CARRY_SLOTS, 1, 600)  # (salt 5: an odd shift, the two are boundary values in turn)
    if index % 4 == 0:  # both on a boundary
        old_cap = CARRY_SLOTS[(index // 4) % len(CARRY_SLOTS)]
    W = PNP_WINDOW_LEN[(index // 2) % 4]
    n = int(rng.integers(1, 7))
    kinds = tuple(_weighted(rng, CARRY_KINDS, (3, 3, 2, 2, 1, 1, 1, 1)) for _ in range(n))
    pairs = [_carry_window(rng, k, W, old_cap, cap) for k in kinds]
    olds, news = [p[0] for p in pairs], [p[1] for p in pairs]
    params = _pnp_params(rng, index)
    K = CR.K
    old_poses, old_tracks, old_seen = CR.stack_old(olds)
    origin, tracks, seen = CR.stack_new(news)
    block = LS.seq_build(seq_lib("lm"), K, old_poses, old_tracks, old_seen)
    # the source: the block's points as built, or (every fourth draw of at most 257 old slots) as solved.  Neither
    # holds a coordinate that is not finite -- the build drops such a landmark, the solve hands its input back when a
    # step fails -- so rule A's finite test is left to tests/test_carry.py's case of the host entry, whose old points are the caller's
    solve, points = None, None
    if index % 4 == 3 and old_cap <= 257:
        solve = dict(delta=BA_DELTA[int(rng.integers(0, 2))], max_iters=int(rng.integers(1, 21)))
        pts3 = [LS.seq_ba(seq_lib("ba"), K, old_poses[w], *(LS.window_of(block, w)[i] for i in (0, 2, 3, 4)),
                          solve["delta"], solve["max_iters"])[1]
                for w in range(n) if block["status"][w] == LR.OK]
        points = np.concatenate(pts3) if pts3 else np.zeros((0, 3))
    carry = CR.join(block, origin, old_cap, points)
    loc = CR.localise(seq_lib("pnp"), carry, tracks, seen, **params)
    return dict(family="carry", seed=seed, index=index, cap=cap, old_cap=old_cap, W=W, kinds=kinds, olds=olds,
                news=news, params=params, K=K, old=(old_poses, old_tracks, old_seen), origin=origin, tracks=tracks,
                seen=seen, solve=solve, points=points, expected=dict(block=block, carry=carry, loc=loc))


def run_carry(c, d):
    pkg = importlib.import_module("visual-odometry-gpu_amd")
    CA = pkg.orbx_carry
    old_poses, old_tracks, old_seen = d["old"]
    c.landmarks_build(d["K"], old_tracks, old_seen, old_poses)
    got = dict(block=c.landmarks_fetch())
    if d["solve"] is not None:
        c.bundle_adjust_landmarks(d["solve"]["delta"], d["solve"]["max_iters"])
    CA.landmarks_carry(c, d["origin"], source=CR.CARRY_BUILT if d["solve"] is None else CR.CARRY_SOLVED)
    got["carry"] = CA.landmarks_carry_fetch(c)
    CA.window_poses_pnp_carried(c, d["K"], d["tracks"], d["seen"], **d["params"])
    got["loc"] = CA.window_poses_pnp_carried_fetch(c)
    return got


def diff_carry(got, exp):
    out = ["block.%s" % k for k in LS.KEYS + ("pose_offset",) if not SS.bits_equal(got["block"][k], exp["block"][k])]
    out += ["carry.%s" % k for k in ("xyz", "point", "count") if not same_bits(got["carry"][k], exp["carry"][k])]
    out += _diff_records(got["loc"]["records"], exp["loc"]["records"], "records")
    out += ["loc.%s" % k for k in ("poses6", "mask", "window_status") if not same_bits(got["loc"][k], exp["loc"][k])]
    return out


# ---- point descriptors and the re-association (rank 19) ----------------------------------------------------------
PD_R = 20  # rule C's reach for every patch_size up to 41


def _reloc_specials(w, h, r=PD_R):
    """test_reloc.case_points' fixed points for a w x h frame: the .5 ties of both parities, R and R - 1 from every
    border, what is not usable"""
    return np.float32([
        (20.5, 20.0), (21.5, 20.0), (20.0, 20.5), (20.0, 21.5), (22.5, 23.5), (r, r), (r - 1, r), (r, r - 1),
        (w - 1 - r, h - 1 - r), (w - r, h - 1 - r), (w - 1 - r, h - r), (w - 1 - r, r), (r, h - 1 - r),
        (w - 1 - r + 0.49, r + 1.0), (w - 1 - r + 0.5, r + 1.0), (w - 1 - r + 0.51, r + 1.0), (r - 0.5, r + 2.0),
        (r - 0.51, r + 2.0), (r + 2.0, h - 1 - r + 0.5), (r + 2.0, h - 1 - r + 0.51), (np.nan, r), (r, np.nan),
        (np.inf, r), (r, -np.inf), (-1.0, r), (r, -0.25), (w - 1.0, h - 1.0), (w - 0.99, r), (r, h - 0.5), (1e9, r),
        (0.0, 0.0), (-0.0, r + 3.0)])


def _reloc_points(rng, n, cap, w, h, near=None):
    """(n, cap, 2) float32: the specials, uniform floats inside rule C's interior and over the whole frame (and a
    little beyond it), and -- with `near`, the points of the other bank -- copies of those, some moved by less than
    half a pixel"""
    sp = _reloc_specials(w, h)
    pts = np.zeros((n, cap, 2), np.float32)
    for f in range(n):
        u = rng.random(cap)
        inside = np.c_[rng.uniform(PD_R - 0.5, w - 1 - PD_R + 0.5, cap), rng.uniform(PD_R - 0.5, h - 1 - PD_R + 0.5, cap)]
        frame = np.c_[rng.uniform(-2.0, w + 1.0, cap), rng.uniform(-2.0, h + 1.0, cap)]
        pts[f] = np.where((u < 0.75)[:, None], inside, frame)
        special = rng.random(cap) < (0.5 if cap <= 5 else 0.2)
        pts[f, special] = sp[rng.integers(0, len(sp), int(special.sum()))]
        if near is not None:
            take = rng.random(cap) < 0.6
            src = near[f, rng.integers(0, near.shape[1], cap)]
            moved = src + np.where(rng.random((cap, 1)) < 0.5, rng.uniform(-0.45, 0.45, (cap, 2)), 0.0).astype(np.float32)
            pts[f, take] = moved[take]
    return pts


def _reloc_bank(rng, index, bank, frames, params, near=None):
    """one orbx_describe_points_device call: points, layout and gates, and rules A-E on the oracle per frame"""
    n, h, w = frames.shape
    cap = RELOC_SLOTS[(index + 3 * bank) % len(RELOC_SLOTS)]
    pts = _reloc_points(rng, n, cap, w, h, near)
    layout = ("pairs", "lk")[int(rng.integers(0, 2))]
    lk = (int(rng.integers(2, 7)), 0)
    lk = (lk[0], int(rng.integers(0, lk[0])))  # (window_len, frame) of an LK-shaped tracks block
    seen_min = int(rng.integers(0, 5))
    seen = rng.integers(0, 6, (n, cap)).astype(np.int32) if seen_min else None
    counts = None
    if rng.random() < 0.6:  # ragged: 0, the capacity, anything between
        counts = np.array([(0, cap, int(rng.integers(0, cap + 1)), int(rng.integers(0, cap + 1)))[int(rng.integers(0, 4))]
                           for _ in range(n)], np.int32)
    ref = [RR.describe_points(frames[f], pts[f], params, seen=None if seen is None else seen[f], seen_min=seen_min,
                              count=None if counts is None else int(counts[f])) for f in range(n)]
    exp = dict(desc=np.stack([r["desc"] for r in ref]), angle=np.stack([r["angle"] for r in ref]),
               state=np.stack([r["state"] for r in ref]), n_ok=np.array([r["n_ok"] for r in ref], np.int32))
    return dict(points=pts, layout=layout, lk=lk, seen=seen, seen_min=seen_min, counts=counts,
                pix=np.stack([r["pix"] for r in ref])), exp


def _ra_sets(rng, kind, n, qcap, tcap):
    """n windows of one kind: (qdesc (n, qcap, 32), qstate, tdesc (n, tcap, 32), tstate)"""
    qdesc = rng.integers(0, 256, (n, qcap, 32), dtype=np.uint8)
    tdesc = rng.integers(0, 256, (n, tcap, 32), dtype=np.uint8)
    qstate = np.full((n, qcap), RR.PD_OK, np.int32)
    tstate = np.full((n, tcap), RR.PD_OK, np.int32)
    for w in range(n):
        if kind == "pool":
            qdesc[w], tdesc[w] = RR.pool_window(rng, qcap, tcap)  # test_matcher.tie_heavy's pool, with matches
        else:  # copies of train slots with 0 .. 60 bits flipped among random descriptors
            for q in np.flatnonzero(rng.random(qcap) < 0.7):
                qdesc[w, q] = RR.flip(tdesc[w, int(rng.integers(0, tcap))], rng, int(rng.integers(0, 61)))
        if kind == "mixed":
            qstate[w] = rng.choice([RR.PD_NONE, RR.PD_BORDER, RR.PD_OK], qcap, p=[0.15, 0.15, 0.7])
            tstate[w] = rng.choice([RR.PD_NONE, RR.PD_BORDER, RR.PD_OK], tcap, p=[0.15, 0.15, 0.7])
        elif kind == "one":
            tstate[w] = rng.choice([RR.PD_NONE, RR.PD_BORDER], tcap)
            tstate[w, int(rng.integers(0, tcap))] = RR.PD_OK
        elif kind == "none":
            tstate[w] = rng.choice([RR.PD_NONE, RR.PD_BORDER], tcap)
    return qdesc, qstate, tdesc, tstate


def draw_reloc(seed, index):
    """Two orbx_describe_points_device calls, one per bank, on one batch of frames, and one re-association: of uploaded
    descriptor sets (orbx_reassociate_device), of the two banks' views (the chain on the device) or of one window of
    host arrays (orbx_reassociate), in turn."""
    rng = _rng("reloc", seed, index)
    context = (index // 4) % len(RELOC_CONTEXTS)
    params = O.gpu_params(**RELOC_CONTEXTS[context])
    w, h = RELOC_WIDTHS[index % len(RELOC_WIDTHS)], RELOC_HEIGHTS[(index // 2) % len(RELOC_HEIGHTS)]
    nf = int(rng.integers(1, 5))
    frames = np.stack([fuzz_parity.image(rng, h, w) for _ in range(nf)])
    # frames as regions of a parent buffer: the row stride equal to the width or above it, garbage in between
    rs = w + (0, int(rng.integers(1, 24)))[int(rng.integers(0, 2))]
    base, fs = int(rng.integers(0, 8)), rs * h + int(rng.integers(0, 50))
    garbage = rng.integers(0, 256, base + nf * fs, dtype=np.uint8)
    b0, e0 = _reloc_bank(rng, index, 0, frames, params)
    b1, e1 = _reloc_bank(rng, index, 1, frames, params, near=b0["points"])
    kind = _weighted(rng, RA_KINDS, (3, 3, 2, 1, 1))
    source = RA_INPUTS[index % 3]
    ra = dict(kind=kind, input=source, ratio=RA_RATIOS[int(rng.integers(0, 3))],
              max_distance=RA_MAX_DISTANCE[int(rng.integers(0, 3))], unique=int(rng.random() < 0.7))
    big = rng.random() < 0.5  # half of the query sets beyond one workgroup of k_ra_knn2
    qcap = (257, 512, 513)[int(rng.integers(0, 3))] if big else RA_CAPS[int(rng.integers(0, len(RA_CAPS)))]
    tcap = RA_CAPS[int(rng.integers(0, len(RA_CAPS)))]
    nw = 1 if source == "host" else int(rng.integers(1, 5))
    sets = _ra_sets(rng, kind, nw, qcap, tcap)
    if source == "banks":  # queries: bank 1, train: bank 0
        ra["kind"] = "described"
        sets = (e1["desc"], e1["state"], e0["desc"], e0["state"])
    ra.update(zip(("qdesc", "qstate", "tdesc", "tstate"), sets))
    exp = dict(banks=[e0, e1], ra=RR.reassociate(*sets, ra["ratio"], ra["max_distance"], ra["unique"]))
    return dict(family="reloc", seed=seed, index=index, context=context, frames=frames, row_stride=rs,
                layout=(base, rs, fs), garbage=garbage, banks=[b0, b1], ra=ra, expected=exp)


_RELOC_CTX = {}


def _close_reloc_context():
    for c in _RELOC_CTX.values():
        c.close()
    _RELOC_CTX.clear()


def reloc_context(pkg, i):
    """RELOC_CONTEXTS[i] opened on CONTEXT's sizes; one is open at a time, the one before is closed first, and
    context(pkg, "reloc") closes the last one when its block ends"""
    if i not in _RELOC_CTX:
        _close_reloc_context()
        _RELOC_CTX[i] = pkg.Context(pkg.default_params("gpu", **dict(CONTEXT, **RELOC_CONTEXTS[i])))
    return _RELOC_CTX[i]


@contextlib.contextmanager
def context(pkg, family):
    """What a sweep or a campaign of `family` runs inside: the one small context of CONTEXT, handed to run() -- or,
    for the reloc family, None: run_reloc opens RELOC_CONTEXTS one after another, and the last one is closed here."""
    if family == "reloc":
        try:
            yield None
        finally:
            _close_reloc_context()
    else:
        with pkg.Context(pkg.default_params("gpu", **CONTEXT)) as c:
            yield c


def run_reloc(c, d):
    """(on the family's own context of the draw; `c` is None under context(pkg, "reloc"))"""
    import torch

    pkg = importlib.import_module("visual-odometry-gpu_amd")
    RL = pkg.orbx_reloc
    c = reloc_context(pkg, d["context"])
    frames = d["frames"]
    nf, h, w = frames.shape
    base, rs, fs = d["layout"]
    buf = d["garbage"].copy()
    np.lib.stride_tricks.as_strided(buf[base:], shape=(nf, h, w), strides=(fs, rs, 1))[...] = frames
    t = torch.as_strided(torch.from_numpy(buf).cuda(), (nf, h, w), (fs, rs, 1), base)
    got = dict(banks=[])
    for bank, b in enumerate(d["banks"]):
        pts = b["points"]
        if b["layout"] == "lk":  # frame k of a tracks block (n, slots, window_len, 2)
            L, k = b["lk"]
            block = np.full((nf, pts.shape[1], L, 2), -7.0, np.float32)
            block[:, :, k] = pts
            xy = torch.from_numpy(block).cuda()[:, :, k]
        else:
            xy = torch.from_numpy(pts).cuda()
        seen = None if b["seen"] is None else torch.from_numpy(b["seen"]).cuda()
        counts = None if b["counts"] is None else torch.from_numpy(b["counts"]).cuda()
        torch.cuda.synchronize()
        RL.describe_points(c, t, xy, bank=bank, seen=seen, seen_min=b["seen_min"], counts=counts)
        if d["ra"]["input"] != "banks":  # (the chain on the device fetches nothing in between)
            got["banks"].append(RL.point_descriptors_fetch(c, bank))
    r = d["ra"]
    if r["input"] == "host":
        one = RL.reassociate_host(c, r["qdesc"][0], r["qstate"][0], r["tdesc"][0], r["tstate"][0], r["ratio"],
                                  r["max_distance"], r["unique"])
        got["ra"] = dict(origin=one["origin"][None], dist=one["dist"][None], count=np.array([one["count"]], np.int32))
    else:
        if r["input"] == "banks":
            RL.reassociate(c, RL.point_descriptors_view(c, 1), train_desc=RL.point_descriptors_view(c, 0),
                           ratio=r["ratio"], max_distance=r["max_distance"], unique=r["unique"])
        else:
            RL.reassociate(c, r["qdesc"], r["qstate"], r["tdesc"], r["tstate"], ratio=r["ratio"],
                           max_distance=r["max_distance"], unique=r["unique"])
        got["ra"] = RL.reassociate_fetch(c)
    if r["input"] == "banks":
        got["banks"] = [RL.point_descriptors_fetch(c, bank) for bank in (0, 1)]
    return got


def diff_reloc(got, exp):
    out = []
    for bank, (g, e) in enumerate(zip(got["banks"], exp["banks"])):
        out += ["bank %d %s" % (bank, k) for k in ("state", "n_ok", "desc", "angle") if not same_bits(g[k], e[k])]
    out += ["re-association %s" % k for k in ("origin", "dist", "count") if not same_bits(got["ra"][k], exp["ra"][k])]
    return out


# ---- the common face ---------------------------------------------------------------------------------------------
_DRAW = dict(matcher=draw_matcher, pose=draw_pose, scale=draw_scale, ba=draw_ba, corners=draw_corners, tracks=draw_tracks, landmarks=draw_landmarks,
             pnp=draw_pnp, carry=draw_carry, reloc=draw_reloc)
_RUN = dict(matcher=run_matcher, pose=run_pose, scale=run_scale, ba=run_ba, corners=run_corners, tracks=run_tracks, landmarks=run_landmarks,
            pnp=run_pnp, carry=run_carry, reloc=run_reloc)
_DIFF = dict(matcher=diff_matcher, pose=diff_pose, scale=diff_scale, ba=diff_ba, corners=diff_corners, tracks=diff_tracks, landmarks=diff_landmarks,
             pnp=diff_pnp, carry=diff_carry, reloc=diff_reloc)


def draw(family, seed, index):
    return _DRAW[family](seed, index)


def run(family, ctx, d):
    return _RUN[family](ctx, d)


def compare(family, got, d):
    """Every fetched array against the expected one, bit for bit; the message names the draw."""
    bad = _DIFF[family](got, d["expected"])
    assert not bad, ((family, d["seed"], d["index"]), bad)


def elements(family, d):
    """what one draw compares: (name, count)"""
    if family == "matcher":
        return "queries", len(d["q"])
    if family == "pose":
        return "correspondences", len(d["p1"])
    if family == "scale":
        return "points", sum(len(t[0]) for t in d["tri"]) + len(d["lists"][0]) + len(d["lists"][1])
    if family == "corners":
        return "frames", 2 * len(d["frames"]) + 1
    if family == "tracks":
        return "pairs", len(d["pairs"])
    if family == "landmarks":
        return "slots", d["seen"].size
    if family == "pnp":
        return "problems", d["expected"]["pnp"]["records"].size
    if family == "carry":
        return "problems", d["expected"]["loc"]["records"].size
    if family == "reloc":
        return "slots", sum(p["points"].size // 2 for p in d["banks"]) + d["ra"]["qstate"].size
    return "windows", len(d["windows"])


def describe(family, d):
    """one line on a draw, for the verbose replay"""
    if family == "matcher":
        return "nq %d nt %d ratio %g kind %s" % (len(d["q"]), len(d["t"]), d["ratio"], d["kind"])
    if family == "pose":
        return "n %d %s outliers %.2f %s K[0,0] %g %r" % (len(d["p1"]), d["variant"], d["outliers"], d["noise"],
                                                          d["K"][0, 0], d["kw"])
    if family == "scale":
        prev, cur, pv, cv = d["lists"]
        return "tri n %d pose %s; lists %s %d / %d flags %s / %s" % (
            len(d["tri"][0][0]), d["pose"], d["kind"], len(prev), len(cur),
            "NULL" if pv is None else int(np.sum(pv)), "NULL" if cv is None else int(np.sum(cv)))
    if family == "corners":
        return "%d frames %dx%d%s%s q %g d %g max %d / masked %d; %d seed slots seen_min %d; mask %s" % (
            d["frames"].shape + (" strided %r" % (d["layout"],) if d["strided"] else "", " blocks" if d["blocks"] else "",
                                 d["quality"], d["dist"], d["max_corners"], d["masked_max"], d["seeds"].shape[1],
                                 d["seen_min"], d["mask_kind"]))
    if family == "tracks":
        return "%d slots, L %d, windows %s, stride %d, align %s, T_start %s, scale0 %g, K[0,0] %g, %r" % (
            d["cap"], d["L"], d["patterns"], d["stride"], d["align"], "NULL" if d["T_start"] is None else "given",
            d["first"], d["K"][0, 0], d["kw"])
    if family == "landmarks":
        return "%d slots, W %d, build %s gate %g, min_seen %d, windows %s, delta %g, max_iters %d" % (
            d["slots"], d["W"], d["build"], d["gate"], d["min_seen"], d["kinds"], d["delta"], d["max_iters"])
    if family == "pnp":
        return "%d slots, W %d, windows %s, %r, host problem %s, seeded solve %s" % (
            d["cap"], d["W"], d["kinds"], d["params"], None if d["host"] is None else (d["host"]["w"], d["host"]["k"]),
            d["solve"])
    if family == "carry":
        return "%d slots from %d old ones, W %d, windows %s, source %s, %r" % (
            d["cap"], d["old_cap"], d["W"], d["kinds"], "built" if d["solve"] is None else "solved %r" % d["solve"],
            d["params"])
    if family == "reloc":
        a, r = d["banks"], d["ra"]
        return ("context %d %r; %d frames %dx%d row stride %d; banks %s; re-association %s of %s: %d windows, %d "
                "queries, %d train slots, ratio %g, max_distance %d, unique %d" % (
                    d["context"], RELOC_CONTEXTS[d["context"]], d["frames"].shape[0], d["frames"].shape[2],
                    d["frames"].shape[1], d["row_stride"],
                    [(p["points"].shape[1], p["layout"], p["seen_min"], "counts" if p["counts"] is not None else "no counts")
                     for p in a], r["kind"], r["input"], len(r["qstate"]), r["qstate"].shape[1], r["tstate"].shape[1],
                    r["ratio"], r["max_distance"], r["unique"]))
    return "%d windows, delta %g, max_iters %d: %s" % (len(d["windows"]), d["delta"], d["max_iters"], d["names"])
