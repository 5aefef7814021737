"""Pose and scale of tracked frame pairs on the CPU (test helper for tests/test_tracks_pose_ref.py and
tests/test_tracks_pose.py).

    tracks_xy[w][slot][k], seen[w][slot]  ->  per pair p = w * (L - 1) + k: slot list, pose, mask, points, scale

restated as: rule 1 (the slot lists) in numpy, then tests/cpp/pose_sequential.cpp on the two point lists,
tests/cpp/scale_sequential.cpp for the points and, from pair 1 of a window on, for the join with the previous pair of
the SAME window, the two slot lists being the join's index arrays.  No arithmetic is restated here: every link is
pinned against numpy by the CPU tests of its own module (tests/chain_ref.py does the same for the matching route).

Also here: the synthetic blocks the GPU tests upload, so that the CPU tests can assert which classes they contain.
"""
import hashlib

import numpy as np

import landmarks_ref as LR
from test_pose import K_ANISO, K_KITTI, seq_pose
from test_scale import seq_join, seq_triangulate

POSE_DEFAULTS = dict(prob=0.999, threshold=1.0, max_iters=1000, seed=0)


def slot_lists(seen, L):
    """Rule 1.  seen: (n_windows, slots) int.  -> per global pair, the slots with clamp(seen, 0, L) >= k + 2, ascending"""
    seen = np.clip(np.asarray(seen, np.int64), 0, L)
    return [np.flatnonzero(seen[w] >= k + 2).astype(np.int32) for w in range(seen.shape[0]) for k in range(L - 1)]


_pose = {}


def _key(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(a.tobytes())
        h.update(str(a.shape).encode())
    return h.hexdigest()


def restate(libs, K, tracks, seen, **pose_kw):
    """libs: (pose restatement, scale restatement), the `seq` fixtures of tests/test_pose.py and tests/test_scale.py.
    tracks (n, slots, L, 2) float32, seen (n, slots).  -> one dict per global pair: w, k, slots, p1, p2, pose (what
    seq_pose returns), xyz, valid, scale, triplets, ratios"""
    pose_lib, scale_lib = libs
    kw = dict(POSE_DEFAULTS, **pose_kw)
    tracks = np.ascontiguousarray(tracks, np.float32)
    n, cap, L, _ = tracks.shape
    lists = slot_lists(np.asarray(seen).reshape(n, cap), L)
    K = np.ascontiguousarray(K, np.float64)
    pairs = []
    for p, slots in enumerate(lists):
        w, k = divmod(p, L - 1)
        p1, p2 = tracks[w, slots, k], tracks[w, slots, k + 1]
        key = (_key(p1, p2, K), tuple(sorted(kw.items())))
        if key not in _pose:
            pose = seq_pose(pose_lib, p1, p2, K, **kw)
            _pose[key] = (pose,) + seq_triangulate(scale_lib, p1, p2, pose["R"], pose["t"], K)
        pose, xyz, valid = _pose[key]
        cur = dict(w=w, k=k, slots=slots, p1=p1, p2=p2, pose=pose, xyz=xyz, valid=valid)
        if k == 0:
            cur.update(scale=1.0, triplets=0, ratios=0)
        else:
            prev = pairs[-1]
            s, trip, used = seq_join(scale_lib, prev["slots"], prev["xyz"], prev["valid"], prev["pose"]["R"],
                                     prev["pose"]["t"], slots, xyz, valid)
            cur.update(scale=s, triplets=len(trip), ratios=used)
        pairs.append(cur)
    return pairs


def block(pairs, cap):
    """The result block of rule 5 as whole arrays, zero past every pair's list"""
    m = len(pairs)
    out = dict(E=np.zeros((m, 9)), R=np.zeros((m, 9)), t=np.zeros((m, 3)), inliers=np.zeros(m, np.int32),
               good=np.zeros(m, np.int32), iters=np.zeros(m, np.int32), n=np.zeros(m, np.int32), scale=np.zeros(m),
               triplets=np.zeros(m, np.int32), ratios_used=np.zeros(m, np.int32), slot_of=np.zeros((m, cap), np.int32),
               mask=np.zeros((m, cap), np.uint8), xyz=np.zeros((m, cap, 3), np.float32),
               valid=np.zeros((m, cap), np.uint8))
    for i, p in enumerate(pairs):
        r, k = p["pose"], len(p["slots"])
        out["E"][i], out["R"][i], out["t"][i] = r["E"].reshape(9), r["R"].reshape(9), r["t"]
        out["inliers"][i], out["good"][i], out["iters"][i], out["n"][i] = r["inliers"], r["good"], r["iters"], k
        out["scale"][i], out["triplets"][i], out["ratios_used"][i] = p["scale"], p["triplets"], p["ratios"]
        out["slot_of"][i, :k], out["mask"][i, :k] = p["slots"], r["mask"]
        out["xyz"][i, :k], out["valid"][i, :k] = p["xyz"], p["valid"]
    return out


def assert_blocks_equal(got, ref):
    """exact equality, floating point by bit pattern"""
    assert set(got) == set(ref)
    for k in ref:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), (k, np.flatnonzero(a.reshape(-1) != b.reshape(-1))[:8])


# ---- true motion of a landmarks_ref.make_scene window ----------------------------------------------------------


def true_pairs(scene):
    """-> per pair k of the window: (R, unit t, |t|) with x_{k+1} = R x_k + t"""
    out = []
    poses = scene["true_poses"]
    for k in range(len(poses) - 1):
        Ra, Rb = LR.rodrigues(poses[k, :3]), LR.rodrigues(poses[k + 1, :3])
        R = Rb @ Ra.T
        t = poses[k + 1, 3:] - R @ poses[k, 3:]
        out.append((R, t / np.linalg.norm(t), float(np.linalg.norm(t))))
    return out


# ---- the synthetic blocks of the GPU tests ---------------------------------------------------------------------

PATTERNS = ("ragged", "all", "second_dead", "dead", "four", "five", "odd_seen", "noisy")


def window(seed, cap, L, pattern, K=K_KITTI):
    """One window of a make_scene whose `seen` follows `pattern`: ragged (uniform in [0, L]), all (every slot seen in
    every frame), second_dead (every second slot never seen), dead (no slot), four / five (that many survivors of all
    pairs, where the slots allow), odd_seen (ragged, with `seen` values above L and below 0 that rule 1 clamps), noisy
    (ragged with 0.3 px noise and 20 % outliers)"""
    full = pattern in ("all", "second_dead", "dead", "four", "five")
    sc = LR.make_scene(seed, W=L, slots=cap, min_seen=L if full else 0, K=K,
                       **(dict(sigma=0.3, outliers=0.2) if pattern == "noisy" else {}))
    tracks, seen = sc["tracks"].copy(), sc["seen"].copy()
    if pattern == "second_dead":
        seen[1::2] = 0
    elif pattern == "dead":
        seen[:] = 0
    elif pattern in ("four", "five"):
        keep = np.flatnonzero(seen == L)[np.linspace(0, (seen == L).sum() - 1, 4 if pattern == "four" else 5).astype(int)] \
            if (seen == L).sum() else np.zeros(0, int)
        keep = np.unique(keep)
        dead = np.ones(cap, bool)
        dead[keep] = False
        seen[dead] = 0
    elif pattern == "odd_seen":
        seen = np.where(seen == L, L + 3, seen)
        seen = np.where(seen == 0, -2, seen)
    if pattern != "odd_seen":
        tracks[np.arange(L)[None, :] >= seen[:, None]] = 0.0  # zero past `seen`, as the tracker leaves them
    return tracks, seen.astype(np.int32)


def case(name, cap, L, patterns, K=K_KITTI, seed0=0, **kw):
    ws = [window(seed0 + 17 * i, cap, L, p, K) for i, p in enumerate(patterns)]
    return dict(name=name, K=K, cap=cap, L=L, tracks=np.stack([w[0] for w in ws]), seen=np.stack([w[1] for w in ws]),
                kw=dict(POSE_DEFAULTS, **kw), patterns=patterns)


def gpu_cases():
    """slot_capacity in {1, 5, 63, 64, 65, 257, 300}, L in {2, 3, 5}, 1 .. 7 windows, max_iters in {0, 33, 1000},
    K_KITTI and K_ANISO, every pattern"""
    return [
        case("cap1", 1, 2, ("all",), max_iters=33),
        case("cap1_L3", 1, 3, ("all", "dead"), max_iters=33),
        case("cap5", 5, 3, ("all", "four"), max_iters=1000),
        case("cap63", 63, 5, ("ragged", "odd_seen", "noisy"), max_iters=33, seed0=3),
        case("cap64", 64, 3, ("all", "all", "ragged", "second_dead"), max_iters=0, seed0=5),
        case("cap65", 65, 2, ("second_dead", "all", "four", "five", "dead"), max_iters=33, seed0=7),
        case("cap257", 257, 5, ("ragged", "all", "second_dead", "dead", "four", "five", "noisy"), max_iters=1000,
             seed0=11),
        case("cap300_aniso", 300, 3, ("all", "odd_seen", "five", "dead", "noisy", "ragged"), K=K_ANISO, max_iters=33,
             seed0=13),
    ]


def classes(pairs):
    """What a restated batch contains, for the CPU test that the GPU inputs cover what they claim"""
    n = np.array([len(p["slots"]) for p in pairs])
    per_window = {}
    for p in pairs:
        per_window.setdefault(p["w"], []).append(len(p["slots"]))
    return dict(
        crosses_64=bool(((n > 64) & (n < 256)).any()), crosses_256=bool((n > 256).any()),
        n0=bool((n == 0).any()), n4=bool((n == 4).any()), n5=bool((n == 5).any()),
        no_ratio=any(p["k"] >= 1 and p["triplets"] >= 1 and p["ratios"] == 0 for p in pairs),
        dead_window=any(max(v) == 0 for v in per_window.values()),
        scaled=any(p["k"] >= 1 and p["ratios"] >= 10 for p in pairs),
        posed=any(p["pose"]["good"] >= 5 for p in pairs))
