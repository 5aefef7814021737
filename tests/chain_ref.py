"""The batched chain on the CPU (test helper for tests/test_batch_chain.py; DESIGN.md §9, "uneven batches").

    batch_host / batch_device -> batch_match_consecutive -> batch_pose_consecutive -> batch_scale_consecutive

restated as: the C oracle's ORB per frame, the oracle's matcher per consecutive pair, tests/cpp/pose_sequential.cpp on
the matched keypoints, tests/cpp/scale_sequential.cpp (triangulation, and from pair 1 on the join with the previous
pair).  Every link is pinned against numpy by the CPU tests of its own module, so the chain gives the expected match
lists, poses, masks, points, valid flags, scales, triplet and ratio counts bit for bit: `check` compares everything a
context offers for its last batch with it, by exact equality.

Also here: the seeded frame generators and the batch sets U, Q, S and H built from them.
"""
import hashlib

import numpy as np

import oracle_lib as O
from test_pose import K_KITTI, H, W, seq_pose, zero_result
from test_scale import seq_join, seq_triangulate

K_1080 = np.array([[1000.0, 0, 960.0], [0, 1000.0, 540.0], [0, 0, 1]])
POSE_DEFAULTS = dict(prob=0.999, threshold=1.0, max_iters=1000, seed=0)
OKW_U = dict(nfeatures=3000)  # the reference's VO loops build cv::ORB::create(3000)
OKW_H = dict(nfeatures=4000, nlevels=12, scale_factor=1.2, blur_levels=2, blur_kind=0)

# ---- frames ------------------------------------------------------------------------------


def flat(h=H, w=W):
    return np.full((h, w), 89, np.uint8)


def few(r, seed, h=H, w=W):
    """r random rectangles on a flat frame (in the manner of sparse_frame in tests/test_batch_inputs.py, anywhere in
    the frame): a handful of keypoints"""
    rng = np.random.default_rng(seed)
    img = flat(h, w)
    for _ in range(r):
        ww, hh = int(rng.integers(24, 70)), int(rng.integers(20, max(21, h // 4)))
        x0, y0 = int(rng.integers(4, w - ww - 4)), int(rng.integers(4, h - hh - 4))
        img[y0:y0 + hh, x0:x0 + ww] = int(rng.choice([20, 40, 160, 230]))
    return img


def rolled(img, dy, dx):
    return np.roll(img, (dy, dx), (0, 1))


def cut(img, cols):
    """img in columns < cols, flat elsewhere"""
    out = flat(*img.shape)
    out[:, :cols] = img[:, :cols]
    return out


def few_sequence(seed, r=16):
    """few(r, seed) and its copies moved by (1, 2), (2, 4) and (3, 6): three pairs of a few matches each"""
    f = few(r, seed)
    return [f, rolled(f, 1, 2), rolled(f, 2, 4), rolled(f, 3, 6)]


# seeds of the four-frame sequences appended to set U and the class each one is there for (asserted by
# tests/test_batch_chain.py::test_cpu_set_u_classes)
FEW_SEEDS = (2, 8, 11, 12)


def set_u():
    """Set U, "uneven": rich, empty and nearly empty frames next to each other (1241 x 376, 3000 features)."""
    k0, k1 = O.load_kitti(0), O.load_kitti(1)
    a, b = few(3, 2), few(16, 3)
    frames = [k0, k1, flat(), k1, flat(), flat(), a, rolled(a, 2, 4), b, rolled(b, 1, 2), cut(k0, 200), cut(k1, 200),
              k0, k1, k0, k1]
    for s in FEW_SEEDS:
        frames += few_sequence(s)
    return frames


def set_u_flat_ends():
    """Set U reversed and rotated so that its two adjacent flat frames (4 and 5) are the first and the last one"""
    rev = set_u()[::-1]
    n = len(rev)
    at = n - 1 - 4  # where frame 4 went
    return rev[at:] + rev[:at]


Q_NFEATURES = {67: 64, 259: 255, 260: 256, 262: 257, 2050: 2047, 2051: 2048}  # nfeatures: keypoints per frame


def set_q():
    k0, k1 = O.load_kitti(0), O.load_kitti(1)
    return [k0, k1, k0]


S_SIZES = [(1000, 300), (643, 200), (1237, 371)]


def set_s(w, h):
    """the top-left w x h regions of set U's frames"""
    return [np.ascontiguousarray(f[:h, :w]) for f in set_u()]


def rich(n):
    k0, k1 = O.load_kitti(0), O.load_kitti(1)
    return [(k0, k1)[i & 1] for i in range(n)]


def set_h(pkg):
    """1920 x 1080, 12 levels, 4000 features: a stream-B frame, its copy moved by (2, 5), flat, the frame, the copy"""
    f0 = pkg.streams.stream_b(1, 1080, 1920)[0]
    f1 = rolled(f0, 2, 5)
    return [f0, f1, flat(1080, 1920), f0, f1]


# ---- the chain ---------------------------------------------------------------------------

_orb, _match, _pose = {}, {}, {}


def _key(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha1(a.tobytes()).hexdigest(), a.shape


def oracle_frame(frame, okw):
    key = (_key(frame), tuple(sorted(okw.items())))
    if key not in _orb:
        r = O.detect_and_compute_gpu(frame, O.gpu_params(**okw))
        r["key"] = key
        _orb[key] = r
    return _orb[key]


def chain(libs, frames, okw, K=K_KITTI, ratio=0.8, **pose_kw):
    """libs: (pose restatement, scale restatement), the `seq` fixtures of tests/test_pose.py and tests/test_scale.py.
    -> dict(frames=[oracle result per frame], pairs=[per consecutive pair: q, t, d (the oracle's matches), pose (what
    seq_pose returns), xyz, valid, scale, triplets, ratios])"""
    pose_lib, scale_lib = libs
    kw = dict(POSE_DEFAULTS, **pose_kw)
    refs = [oracle_frame(f, okw) for f in frames]
    Kkey = _key(np.asarray(K, np.float64))
    pairs = []
    for i in range(len(frames) - 1):
        a, b = refs[i], refs[i + 1]
        mk = (a["key"], b["key"], ratio)
        if mk not in _match:
            _match[mk] = O.match_ratio(a["desc"], b["desc"], ratio)
        q, t, d = _match[mk]
        p1, p2 = a["kps"][q].astype(np.float32), b["kps"][t].astype(np.float32)
        pk = (mk, Kkey, tuple(sorted(kw.items())))
        if pk not in _pose:
            pose = seq_pose(pose_lib, p1, p2, K, **kw)
            xyz, valid = seq_triangulate(scale_lib, p1, p2, pose["R"], pose["t"], K)
            _pose[pk] = (pose, xyz, valid)
        pose, xyz, valid = _pose[pk]
        cur = dict(q=q, t=t, d=d, pose=pose, xyz=xyz, valid=valid, nq=len(a["kps"]), nt=len(b["kps"]))
        if i == 0:
            cur.update(scale=1.0, triplets=0, ratios=0)
        else:
            prev = pairs[-1]
            s, trip, used = seq_join(scale_lib, prev["t"], prev["xyz"], prev["valid"], prev["pose"]["R"],
                                     prev["pose"]["t"], q, xyz, valid)
            cur.update(scale=s, triplets=len(trip), ratios=used)
        pairs.append(cur)
    return dict(frames=refs, pairs=pairs)


def is_zero_pose(pair):
    return zero_result(pair["pose"], len(pair["q"]))


def table(ref):
    """one line per pair: what DESIGN.md §9 quotes"""
    lines = ["pair   nq   nt  matches  inliers  good  iters  triplets  ratios  scale"]
    for i, p in enumerate(ref["pairs"]):
        r = p["pose"]
        lines.append("%4d %4d %4d %8d %8d %5d %6d %9d %7d  %.6g" % (i, p["nq"], p["nt"], len(p["q"]), r["inliers"],
                                                                  r["good"], r["iters"], p["triplets"], p["ratios"],
                                                                  p["scale"]))
    return "\n".join(lines)


# ---- the checker -------------------------------------------------------------------------


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _bits1(x):
    return int(np.float64(x).view(np.uint64))


def run_chain(c, K=K_KITTI, ratio=0.8, **pose_kw):
    """match -> pose -> scale on the context's last batch"""
    c.batch_match_consecutive(ratio)
    c.batch_pose_consecutive(K, **dict(POSE_DEFAULTS, **pose_kw))
    c.batch_scale_consecutive(K)


def check(c, ref, w=W, h=H):
    """Everything the context offers for its last batch (detected, matched, posed and scaled) against `ref`
    (what `chain` returned for the same frames and arguments): exact equality throughout."""
    refs, pairs = ref["frames"], ref["pairs"]
    n = len(refs)
    cap = c.plan(w, h)["out_capacity"]
    res = c.batch_fetch(0, n, cap)
    for i, r in enumerate(refs):
        m = int(res["counts"][i])
        assert m == len(r["kps"]), (i, m, len(r["kps"]))
        assert np.array_equal(res["kps"][i, :m], r["kps"]), i
        assert np.array_equal(res["levels"][i, :m], r["levels"]), i
        assert np.array_equal(res["desc"][i, :m] & r["valid"], r["desc"] & r["valid"]), i
    poses = c.batch_pose_fetch()
    scales = c.batch_scale_fetch()
    assert len(poses["iters"]) == len(scales["scale"]) == n - 1
    for i, p in enumerate(pairs):
        q, t, d = c.batch_match_fetch(i, cap)
        assert np.array_equal(q, p["q"]) and np.array_equal(t, p["t"]) and np.array_equal(d, p["d"]), i
        r = p["pose"]
        for k in ("E", "R", "t"):
            assert np.array_equal(_bits(poses[k][i]), _bits(r[k])), (i, k, poses[k][i], r[k])
        got = (int(poses["inliers"][i]), int(poses["good"][i]), int(poses["iters"][i]))
        assert got == (r["inliers"], r["good"], r["iters"]), (i, got)
        mask = c.batch_pose_mask(i)
        assert len(mask) == len(p["q"]) and np.array_equal(mask, r["mask"]), i
        xyz, valid = c.batch_points_fetch(i)
        assert xyz.dtype == np.float32 and xyz.shape == p["xyz"].shape, i
        assert xyz.tobytes() == p["xyz"].tobytes() and np.array_equal(valid, p["valid"]), i
        got = (_bits1(scales["scale"][i]), int(scales["triplets"][i]), int(scales["ratios_used"][i]))
        assert got == (_bits1(p["scale"]), p["triplets"], p["ratios"]), (i, scales["scale"][i], got, p["scale"])
    return len(pairs)
