"""numpy restatement of the landmarks carry (include/orbx_carry.h) and the synthetic streams of
tests/test_carry_ref.py, tests/test_carry.py and tests/test_cpp_carry.py.

The join (rule A) and the gather (rule B) are integer logic and an exact float32 -> float64 widening, restated here with
numpy.searchsorted and boolean masks; each problem's solve (rule C) is rank 17's sequential restatement
tests/cpp/pnp_sequential.cpp through pnp_seq.problem with the problem's seed; status and fill (rules D, E) are numpy.
Nothing here shares code with the library."""
import math

import numpy as np

import landmarks_ref as L
import pnp_seq as S

K = L.K_KITTI
CARRY_BUILT, CARRY_SOLVED = 0, 1
CARRY_OK, CARRY_LOST = 0, 1


# ---- rules A - E ----------------------------------------------------------------------------------------------------
def join(block, origin, old_cap, points=None):
    """Rule A on a fetched landmarks block (Context.landmarks_fetch's dict, or landmarks_seq.seq_build's).  origin:
    (n, cap) int32; points: the source coordinates in the block's order (None: the block's points3 as built).
    Returns dict of xyz (n, cap, 3), point (n, cap) int32, count (n) int32."""
    origin = np.asarray(origin, np.int32)
    n, cap = origin.shape
    src = np.asarray(block["points3"] if points is None else points, np.float64).reshape(-1, 3)
    xyz, point = np.zeros((n, cap, 3)), np.full((n, cap), -1, np.int32)
    for w in range(n):
        if block["status"][w] != L.OK:
            continue
        p0, p1 = int(block["point_offset"][w]), int(block["point_offset"][w + 1])
        slots = np.asarray(block["slot_of_point"][p0:p1])
        assert np.all(np.diff(slots) > 0)  # the slots of a window ascend
        for s in range(cap):
            o = int(origin[w, s])
            if o < 0 or o >= old_cap:
                continue
            j = int(np.searchsorted(slots, o))
            if j < len(slots) and slots[j] == o and np.all(np.isfinite(src[p0 + j])):
                xyz[w, s], point[w, s] = src[p0 + j], j
    return dict(xyz=xyz, point=point, count=(point >= 0).sum(axis=1).astype(np.int32))


def gather(carry, tracks, seen, w, k):
    """Rule B: (slots, world points (m, 3), pixels (m, 2) float64) of problem (w, k), in ascending slot order."""
    W = tracks.shape[2]
    live = np.clip(np.asarray(seen[w], np.int64), 0, W) > k
    px = np.asarray(tracks[w, :, k], np.float32)
    take = (carry["point"][w] >= 0) & live & np.isfinite(px).all(axis=1)
    slots = np.flatnonzero(take)
    return slots, carry["xyz"][w, slots], px[slots].astype(np.float64)


def fill(records):
    """Rule E: (poses6 (n, W, 6), window_status (n))."""
    n, W = records.shape
    poses, status = np.zeros((n, W, 6)), np.zeros(n, np.int32)
    for w in range(n):
        if records["status"][w, 0] != S.OK or records["status"][w, 1] != S.OK:
            status[w] = CARRY_LOST
            continue
        for k in range(W):
            poses[w, k] = records["pose6"][w, k] if records["status"][w, k] == S.OK else poses[w, k - 1]
    return poses, status


def localise(lib, carry, tracks, seen, Kmat=K, **params):
    """Rules B - E on a carry block: dict of records (n, W), poses6 (n, W, 6), mask (n, W, cap), window_status (n)."""
    tracks, seen = np.asarray(tracks, np.float32), np.asarray(seen, np.int32)
    n, cap, W = tracks.shape[:3]
    rec, mask = np.zeros((n, W), S.RECORD), np.zeros((n, W, cap), np.uint8)
    p = dict(S.DEFAULTS, **params)
    for w in range(n):
        for k in range(W):
            if carry["count"][w] == 0:
                rec[w, k]["status"] = S.SKIPPED
                continue
            slots, X, px = gather(carry, tracks, seen, w, k)
            one = S.problem(lib, Kmat, X, px, **dict(p, seed=lib.seq_pnp_problem_seed(p["seed"], k)))
            r = rec[w, k]
            r["pose6"], r["inliers"], r["iters"], r["n_corr"] = one["pose6"], one["inliers"], one["iters"], one["n_corr"]
            r["status"], r["rms_px"] = one["status"], one["rms_px"]
            mask[w, k, slots] = one["mask"]
    poses, status = fill(rec)
    return dict(records=rec, poses6=poses, mask=mask, window_status=status)


# ---- streams ----------------------------------------------------------------------------------------------------------
def make_stream(seed, n_frames, n_points, step=(0.3, 0.6), depth=(8.0, 40.0)):
    """One camera on a gently turning path of n_frames frames (steps of `step` units, at most 2 degrees per step) and
    n_points world points at `depth` in front of camera 0.  Returns dict of poses (n_frames, 6: angle-axis, translation,
    world -> camera, frame 0 the identity), X (n_points, 3) and pix (n_points, n_frames, 2) float32."""
    rng = np.random.default_rng(seed)
    Rwc, c = [np.eye(3)], [np.zeros(3)]
    for _ in range(n_frames - 1):
        a = np.array([rng.uniform(-0.3, 0.3), 1.0, rng.uniform(-0.3, 0.3)])
        dR = L.rodrigues(a / np.linalg.norm(a) * math.radians(rng.uniform(-2.0, 2.0)))
        d = np.array([rng.uniform(-0.05, 0.05), rng.uniform(-0.02, 0.02), 1.0])
        c.append(c[-1] + Rwc[-1] @ (d / np.linalg.norm(d) * rng.uniform(*step)))
        Rwc.append(Rwc[-1] @ dR)
    poses = np.array([np.r_[L.rotvec(R.T), -R.T @ x] for R, x in zip(Rwc, c)])
    pix = np.c_[rng.uniform(0, L.IMG_W, n_points), rng.uniform(0, L.IMG_H, n_points), np.ones(n_points)]
    X = (np.linalg.inv(K) @ pix.T).T * rng.uniform(*depth, n_points)[:, None]
    return dict(poses=poses, X=X, pix=project(poses, X).astype(np.float32))


def project(poses, X):
    """pixels (len(X), len(poses), 2) of world points under world -> camera angle-axis poses"""
    out = np.zeros((len(X), len(poses), 2))
    for k, p in enumerate(poses):
        q = X @ L.rodrigues(p[:3]).T + p[3:]
        out[:, k, 0] = K[0, 0] * q[:, 0] / q[:, 2] + K[0, 2]
        out[:, k, 1] = K[1, 1] * q[:, 1] / q[:, 2] + K[1, 2]
    return out


def window(stream, first, W, ids, seen, cap=None):
    """The window over frames first .. first + W - 1 whose slot s tracks point ids[s] through seen[s] frames: dict of
    tracks (cap, W, 2) float32 (zero past `seen`, as the windows tracker leaves them), seen (cap) int32, ids and
    true_poses (W, 6).  cap: slots, padded with seen = 0."""
    ids, seen = np.asarray(ids, np.int64), np.asarray(seen, np.int32)
    cap = len(ids) if cap is None else cap
    tracks, full = np.zeros((cap, W, 2), np.float32), np.zeros(cap, np.int32)
    live = np.arange(W)[None, :] < seen[:, None]
    tracks[:len(ids)] = np.where(live[..., None], stream["pix"][ids, first:first + W], np.float32(0))
    full[:len(ids)] = seen
    return dict(tracks=tracks, seen=full, ids=ids, true_poses=stream["poses"][first:first + W].copy())


def successor(stream, old, first, W, fresh_ids, seen=None, cap=None):
    """The window that follows `old` (whose last frame is `first`): its slots are a compaction of the old slots that
    were live in the old window's last frame, followed by fresh points with origin -1.  Returns the window with
    origin (cap) int32 (-1 in the padding)."""
    Wold = old["tracks"].shape[1]
    alive = np.flatnonzero(old["seen"][:len(old["ids"])] == Wold)
    ids = np.r_[old["ids"][alive], np.asarray(fresh_ids, np.int64)]
    new = window(stream, first, W, ids, np.full(len(ids), W, np.int32) if seen is None else seen, cap)
    origin = np.full(len(new["seen"]), -1, np.int32)
    origin[:len(alive)] = alive
    new["origin"] = origin
    return new


def two_generations(seed, W=4, old_slots=80, fresh=10, min_seen=2, cap=None):
    """An old window over frames 0 .. W - 1 (seen uniform in [min_seen, W]) and its successor over frames
    W - 1 .. 2 W - 2, every slot of which is seen in all W frames: (stream, old, new)."""
    stream = make_stream(seed, 2 * W - 1, old_slots + fresh)
    rng = np.random.default_rng(seed + 1000)
    old = window(stream, 0, W, np.arange(old_slots), rng.integers(min_seen, W + 1, old_slots))
    new = successor(stream, old, W - 1, W, old_slots + np.arange(fresh), cap=cap)
    return stream, old, new


def scaled(poses, factor):
    """world -> camera poses whose camera centres are `factor` times as far from the world origin"""
    out = np.array(poses, float)
    out[..., 3:] *= factor
    return out


def relative(pa, pb):
    """(R, t) of camera b in camera a's frame, from two world -> camera poses"""
    Ra, Rb = L.rodrigues(pa[:3]), L.rodrigues(pb[:3])
    R = Rb @ Ra.T
    return R, pb[3:] - R @ pa[3:]


def rot_angle(Ra, Rb):
    return 2.0 * math.asin(min(1.0, np.linalg.norm(Ra - Rb) / (2.0 * math.sqrt(2.0))))


# ---- the mixed batch of tests/test_carry.py, checked without a GPU by tests/test_carry_ref.py --------------------------
MIX_W, MIX_CAP = 4, 300
MIX_PARAMS = dict(prob=0.99, threshold_px=0.5, max_iters=300, seed=17, refine_iters=10, min_inliers=4)


def _pad_old(old, cap=MIX_CAP):
    n, W = old["tracks"].shape[:2]
    old["tracks"] = np.concatenate([old["tracks"], np.zeros((cap - n, W, 2), np.float32)])
    old["seen"] = np.concatenate([old["seen"], np.zeros(cap - n, np.int32)])
    old["poses"] = old["true_poses"].copy()
    return old


def _custom(stream, old, origin, ids, seen=None):
    """a successor of `old` with the given origin and point ids"""
    W = MIX_W
    new = window(stream, W - 1, W, ids, np.full(len(ids), W, np.int32) if seen is None else seen, MIX_CAP)
    new["origin"] = np.full(MIX_CAP, -1, np.int32)
    new["origin"][:len(origin)] = origin
    return new


def mixed_batch():
    """(old windows, new windows) of the one mixed batch; what each window is there for: check_mixed."""
    W, rng = MIX_W, np.random.default_rng(5)
    olds, news = [], []
    # 0: clean, 65 carried slots and 10 fresh ones
    st, old, new = two_generations(100, W, 65, 10, min_seen=W, cap=MIX_CAP)
    olds.append(_pad_old(old)), news.append(new)
    # 1: 300 carried slots, 30 % of their pixels replaced
    st, old, new = two_generations(101, W, 300, 0, min_seen=W, cap=MIX_CAP)
    bad = rng.random((300, W)) < 0.3
    junk = np.stack([rng.uniform(0, L.IMG_W, (300, W)), rng.uniform(0, L.IMG_H, (300, W))], axis=-1).astype(np.float32)
    new["tracks"] = np.where(bad[..., None], junk, new["tracks"])
    new["outlier"] = bad
    olds.append(_pad_old(old)), news.append(new)
    # 2: an origin of every kind.  Old slots with seen < 2 own no landmark
    st = make_stream(102, 2 * W - 1, 140)
    old = window(st, 0, W, np.arange(100), np.r_[[W, 0, 1], rng.integers(0, W + 1, 96), [W]])
    none = [1, 2]                                # old slots that own no landmark
    kept = np.flatnonzero(old["seen"] >= 2)      # (the clean scene keeps every one of them)
    origin = np.r_[[kept[0], kept[-1], -1, MIX_CAP, MIX_CAP + 5, none[0], none[1], -7, 2 ** 31 - 1], kept[5:45]]
    ids = np.r_[[kept[0], kept[-1], 100, 101, 102, none[0], none[1], 103, 104], kept[5:45]]
    olds.append(_pad_old(old)), news.append(_custom(st, old, origin, ids))
    # 3: the old window's baseline is below the build's gate
    st, old, new = two_generations(103, W, 65, 10, min_seen=W, cap=MIX_CAP)
    old = _pad_old(old)
    old["poses"][1, 3:] = old["poses"][0, 3:] + np.array([0.01, 0.0, 0.02])
    olds.append(old), news.append(new)
    # 4: three carried slots
    st, old, new = two_generations(104, W, 65, 10, min_seen=W, cap=MIX_CAP)
    new["origin"][3:] = -1
    olds.append(_pad_old(old)), news.append(new)
    # 5: every pixel of frame 2 is random
    st, old, new = two_generations(105, W, 10, 0, min_seen=W, cap=MIX_CAP)
    new["tracks"][:10, 2] = np.c_[rng.uniform(0, L.IMG_W, 10), rng.uniform(0, L.IMG_H, 10)]
    olds.append(_pad_old(old)), news.append(new)
    # 6: seen of 1 .. 4 in the new window
    st = make_stream(106, 2 * W - 1, 100)
    old = window(st, 0, W, np.arange(100), np.full(100, W))
    new = successor(st, old, W - 1, W, [], seen=1 + np.arange(100) % W, cap=MIX_CAP)
    olds.append(_pad_old(old)), news.append(new)
    # 7: two new slots share an origin
    st = make_stream(107, 2 * W - 1, 40)
    old = window(st, 0, W, np.arange(40), np.full(40, W))
    o = np.r_[np.arange(40), [7]]
    olds.append(_pad_old(old)), news.append(_custom(st, old, o, o))
    return olds, news


def stack_old(olds):
    return (np.stack([o["poses"] for o in olds]), np.stack([o["tracks"] for o in olds]),
            np.stack([o["seen"] for o in olds]))


def stack_new(news):
    return (np.stack([n["origin"] for n in news]), np.stack([n["tracks"] for n in news]),
            np.stack([n["seen"] for n in news]))


def check_mixed(block, carry, ref, news):
    """Conditions on the REFERENCE: every window of the mixed batch is what it is there for."""
    W = MIX_W
    st, n, cnt = ref["records"]["status"], ref["records"]["n_corr"], carry["count"]
    ok = [S.OK] * W
    # 0: clean
    assert cnt[0] == 65 and list(st[0]) == ok and (n[0] == 65).all() and (ref["records"]["inliers"][0] == 65).all()
    assert (carry["point"][0, 65:] == -1).all() and ref["window_status"][0] == CARRY_OK
    # 1: more than 256 correspondences, 30 % outliers
    assert cnt[1] == 300 and list(st[1]) == ok and (n[1] == 300).all()
    inl = ref["records"]["inliers"][1]
    assert (inl > 0.6 * 300).all() and (inl < 0.8 * 300).all()
    for k in range(W):  # the mask is the complement of the replaced pixels
        assert np.array_equal(ref["mask"][1, k].astype(bool), ~news[1]["outlier"][:, k]), k
    # 2: an origin of every kind, in a window that is not window 0
    p0, p1 = block["point_offset"][2], block["point_offset"][3]
    assert p0 > 0 and list(carry["point"][2, :9]) == [0, p1 - p0 - 1, -1, -1, -1, -1, -1, -1, -1]
    assert (carry["point"][2, 9:49] >= 0).all() and cnt[2] == 42 and list(st[2]) == ok
    assert not carry["xyz"][2, 2:9].any() and carry["xyz"][2, 0].tobytes() == block["points3"][p0].tobytes()
    assert carry["xyz"][2, 1].tobytes() == block["points3"][p1 - 1].tobytes()
    # 3: the old window is BASELINE
    assert block["status"][3] == L.BASELINE and cnt[3] == 0 and (st[3] == S.SKIPPED).all()
    assert ref["window_status"][3] == CARRY_LOST and not ref["poses6"][3].any()
    # 4: three carried slots
    assert cnt[4] == 3 and (st[4] == S.FEW_POINTS).all() and (n[4] == 3).all()
    assert ref["window_status"][4] == CARRY_LOST
    # 5: frame 2 finds no model and keeps the pose of frame 1
    assert list(st[5]) == [S.OK, S.OK, S.NO_MODEL, S.OK] and ref["records"]["iters"][5, 2] == MIX_PARAMS["max_iters"]
    assert ref["window_status"][5] == CARRY_OK and ref["poses6"][5, 2].tobytes() == ref["poses6"][5, 1].tobytes()
    assert ref["poses6"][5, 1].tobytes() == ref["records"]["pose6"][5, 1].tobytes()
    assert not ref["records"]["pose6"][5, 2].any() and ref["poses6"][5, 1].any()
    # 6: seen of 1 .. 4 thin the problems out
    assert list(n[6]) == [100, 75, 50, 25] and list(st[6]) == ok
    # 7: both slots of one origin are carried
    assert cnt[7] == 41 and carry["point"][7, 40] == carry["point"][7, 7] >= 0 and list(st[7]) == ok
    assert carry["xyz"][7, 40].tobytes() == carry["xyz"][7, 7].tobytes() and (n[7] == 41).all()
    # every record that is not OK is empty
    bad = st != S.OK
    assert not ref["records"]["pose6"][bad].any() and not ref["records"]["inliers"][bad].any()
    assert not ref["records"]["rms_px"][bad].any() and not ref["mask"][bad].any()


# ---- what the carry buys: generations of streams whose first map is `factor` times too large ---------------------------
def scale_streams(n_streams=2, W=4, slots=60, gens=3, dying=10, seed=300, extra_frames=0, streams=None):
    """wins[g][i]: generation g of stream i.  Every window has `slots` slots; `dying` of them end inside the window and
    are replaced by fresh points in the next one.  extra_frames: frames of the stream behind the last generation;
    streams: a list the streams themselves are appended to."""
    wins = [[] for _ in range(gens)]
    for i in range(n_streams):
        st = make_stream(seed + i, gens * (W - 1) + 1 + extra_frames, slots + (gens - 1) * dying)
        if streams is not None:
            streams.append(st)
        seen = np.r_[np.full(slots - dying, W), 2 + np.arange(dying) % (W - 2)]
        wins[0].append(window(st, 0, W, np.arange(slots), seen))
        for g in range(1, gens):
            fresh = slots + (g - 1) * dying + np.arange(dying)
            wins[g].append(successor(st, wins[g - 1][i], g * (W - 1), W, fresh, seen=seen))
    return wins


def cpu_generations(lm_lib, pnp_lib, wins, factor, **params):
    """The chain carry -> carried PnP -> carried build on the CPU restatements (join and localise here,
    landmarks_seq.seq_build), generation 0 built from the true poses scaled by `factor`: the localise dict of every
    generation >= 1."""
    import landmarks_seq as LS

    cap = len(wins[0][0]["seen"])
    poses = np.stack([scaled(w["true_poses"], factor) for w in wins[0]])
    out = []
    for g in range(len(wins)):
        tracks, seen = np.stack([w["tracks"] for w in wins[g]]), np.stack([w["seen"] for w in wins[g]])
        if g > 0:
            carry = join(block, np.stack([w["origin"] for w in wins[g]]), cap)
            out.append(localise(pnp_lib, carry, tracks, seen, **params))
            poses = out[-1]["poses6"]
        block = LS.seq_build(lm_lib, K, poses, tracks, seen)
    return out


def scale_deviation(results, wins, factor):
    """Worst deviations of generations >= 1 from the truth in the map that is `factor` times too large: (|relative
    translation| / (factor |true one|) - 1 over every pair, the angle between the relative rotation and the true one
    over every pair, and the rotation and translation error of every window's frame 0 against the true pose of that
    frame, which is the previous window's last)."""
    ratio = rot = rot0 = t0 = 0.0
    for g, res in enumerate(results, start=1):
        for i, w in enumerate(wins[g]):
            assert res["window_status"][i] == CARRY_OK and (res["records"]["status"][i] == S.OK).all()
            got, true = res["poses6"][i], w["true_poses"]
            for k in range(len(true) - 1):
                R, t = relative(got[k], got[k + 1])
                Rt, tt = relative(true[k], true[k + 1])
                ratio = max(ratio, abs(np.linalg.norm(t) / (factor * np.linalg.norm(tt)) - 1.0))
                rot = max(rot, rot_angle(R, Rt))
            rot0 = max(rot0, rot_angle(L.rodrigues(got[0, :3]), L.rodrigues(true[0, :3])))
            t0 = max(t0, float(np.linalg.norm(got[0, 3:] - factor * true[0, 3:])))
    return ratio, rot, rot0, t0
