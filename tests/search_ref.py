"""numpy restatement of the search by projection (include/orbx_search.h) and the scenes its tests
share.  Independent of the library: the projection (rules P1-P5) from numpy's own Rodrigues formula with np.sin and
np.cos, the gated re-association (rules K-N, I, J) as plain loops over slots with the bit-count table of
tests/reassoc_ref.py."""
import numpy as np

import carry_ref as CR
import landmarks_ref as L
import reassoc_ref as R

PROJ_NONE, PROJ_BEHIND, PROJ_OUTSIDE, PROJ_OK = 0, 1, 2, 3
PD_OK = R.PD_OK
MAX_THETA = 1.0e5


# ---- rules P1-P5 ------------------------------------------------------------------------------------------------------
def rodrigues(a):
    """exp of the angle-axis vector a, in closed form (elementwise numpy only: A A = a a^T - |a|^2 I)"""
    a = np.asarray(a, np.float64)
    th = float(np.sqrt(a @ a))
    A = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    if th == 0.0:
        return np.eye(3)
    return np.eye(3) + (np.sin(th) / th) * A + ((1.0 - np.cos(th)) / (th * th)) * (np.outer(a, a) - (th * th) * np.eye(3))


def pose_accepted(pose6):
    pose6 = np.asarray(pose6, np.float64)
    return bool(np.isfinite(pose6).all() and np.sqrt(pose6[:3] @ pose6[:3]) <= MAX_THETA)


def project_window(points3, slot_of_point, ok, pose6, K, width, height, margin_px, cap, detail=None):
    """Rules P1-P5 of one old window: points3 (n, 3), the ascending slot_of_point (n), ok: the window is ORBX_LM_OK.
    Returns (xy (cap, 2), depth (cap), state (cap) int32, count).  detail: a list that receives, per landmark that
    reaches rule P3, (slot, u, v, depth) before the state is decided -- what boundary_distance measures."""
    xy, depth, state = np.zeros((cap, 2)), np.zeros(cap), np.zeros(cap, np.int32)
    if not ok or not pose_accepted(pose6):
        return xy, depth, state, 0
    Rm, t = rodrigues(pose6[:3]), np.asarray(pose6[3:], np.float64)
    fx, fy, cx, cy = K[0][0], K[1][1], K[0][2], K[1][2]
    seen = set()
    for X, s in zip(np.asarray(points3, np.float64).reshape(-1, 3), np.asarray(slot_of_point).reshape(-1)):
        s = int(s)
        if s < 0 or s >= cap or s in seen:
            continue
        seen.add(s)
        if not np.isfinite(X).all():
            continue
        p = Rm[:, 0] * X[0] + Rm[:, 1] * X[1] + Rm[:, 2] * X[2] + t
        with np.errstate(all="ignore"):
            u, v = (fx * p[0] / p[2] + cx, fy * p[1] / p[2] + cy) if p[2] != 0 else (np.inf, np.inf)
        if detail is not None:
            detail.append((s, u, v, p[2]))
        if not p[2] > 0:
            state[s] = PROJ_BEHIND
        elif (np.isfinite(u) and np.isfinite(v) and -margin_px <= u <= width - 1 + margin_px and
              -margin_px <= v <= height - 1 + margin_px):
            state[s], xy[s], depth[s] = PROJ_OK, (u, v), p[2]
        else:
            state[s] = PROJ_OUTSIDE
    return xy, depth, state, int((state == PROJ_OK).sum())


def project(block, poses6, K, width, height, margin_px, cap, points=None, detail=None):
    """The batch on a fetched landmarks block (Context.landmarks_fetch's dict): poses6 (n, 6), points: the source
    coordinates in the block's order (None: as built).  dict of xy (n, cap, 2), depth (n, cap), state (n, cap) int32
    and count (n) int32."""
    n = len(block["status"])
    src = np.asarray(block["points3"] if points is None else points, np.float64).reshape(-1, 3)
    res = []
    for w in range(n):
        p0, p1 = int(block["point_offset"][w]), int(block["point_offset"][w + 1])
        one = [] if detail is not None else None
        res.append(project_window(src[p0:p1], block["slot_of_point"][p0:p1], block["status"][w] == L.OK, poses6[w], K,
                                  width, height, margin_px, cap, one))
        if detail is not None:
            detail.append(one)
    return dict(xy=np.stack([r[0] for r in res]), depth=np.stack([r[1] for r in res]),
                state=np.stack([r[2] for r in res]), count=np.array([r[3] for r in res], np.int32))


def boundary_distance(detail, width, height, margin_px):
    """The smallest distance of any landmark of project()'s detail to a state boundary: depth 0, and for the landmarks
    in front of the camera the four margin lines."""
    best = np.inf
    for one in detail:
        for _, u, v, z in one:
            best = min(best, abs(z))
            if z > 0:
                best = min(best, abs(u + margin_px), abs(u - (width - 1 + margin_px)), abs(v + margin_px),
                           abs(v - (height - 1 + margin_px)))
    return best


# ---- rules K-N, I, J ----------------------------------------------------------------------------------------------------
def gate_candidates(qxy, txy, radius_px):
    """rule L's test of one float query against double train positions (m, 2): a bool (m); every operation is one
    binary64 operation of numpy's, rounded once"""
    qx, qy = np.float64(np.float32(qxy[0])), np.float64(np.float32(qxy[1]))
    txy = np.asarray(txy, np.float64).reshape(-1, 2)
    r2 = np.float64(radius_px) * np.float64(radius_px)
    with np.errstate(all="ignore"):
        dx, dy = qx - txy[:, 0], qy - txy[:, 1]
        return dx * dx + dy * dy <= r2


def reassociate_gated_window(qdesc, qstate, qxy, tdesc, tstate, txy, tpstate=None, radius_px=20.0, ratio=0.8,
                             max_distance=256, accept_lone=0, unique=1):
    """Rules F, K-N, I, J of one window: (origin (nq), dist (nq), count, candidates (nq)), int32."""
    nq = len(qstate)
    qxy = np.asarray(qxy, np.float32).reshape(-1, 2)
    txy = np.asarray(txy, np.float64).reshape(-1, 2)
    tdesc, tstate = np.asarray(tdesc, np.uint8).reshape(-1, 32), np.asarray(tstate)
    t_in = (tstate == PD_OK) & np.isfinite(txy).all(axis=1)  # rules F and K
    if tpstate is not None:
        t_in &= np.asarray(tpstate) == PROJ_OK
    t_in = np.flatnonzero(t_in)
    origin, dist, cand = np.full(nq, -1, np.int32), np.full(nq, -1, np.int32), np.zeros(nq, np.int32)
    for q in range(nq):
        if qstate[q] != PD_OK or not np.isfinite(qxy[q]).all() or len(t_in) == 0:
            continue
        inside = t_in[gate_candidates(qxy[q], txy[t_in], radius_px)]
        cand[q] = len(inside)
        if len(inside) == 0:
            continue
        d = R.hamming(qdesc[q], tdesc[inside])
        order = np.lexsort((inside, d))  # rule M: by distance, then by slot
        j1, d1 = int(inside[order[0]]), int(d[order[0]])
        if len(inside) >= 2:
            d2 = int(d[order[1]])
            ok = float(np.float32(d1)) < ratio * float(np.float32(d2)) and d1 <= max_distance
        else:
            ok = bool(accept_lone) and d1 <= max_distance
        if ok:
            origin[q], dist[q] = j1, d1
    if unique:
        for t in set(origin[origin >= 0].tolist()):
            qs = np.flatnonzero(origin == t)
            keep = min(qs, key=lambda q: (dist[q], q))
            for q in qs:
                if q != keep:
                    origin[q], dist[q] = -1, -1
    return origin, dist, int((origin >= 0).sum()), cand


def reassociate_gated(qdesc, qstate, qxy, tdesc, tstate, txy, tpstate=None, **params):
    """The batch: dict of origin, dist, candidates (n, qcap) int32 and count (n) int32.  tpstate: None, or (n, tcap)."""
    res = [reassociate_gated_window(qdesc[w], qstate[w], qxy[w], tdesc[w], tstate[w], txy[w],
                                    None if tpstate is None else tpstate[w], **params) for w in range(len(qdesc))]
    return dict(origin=np.stack([r[0] for r in res]), dist=np.stack([r[1] for r in res]),
                count=np.array([r[2] for r in res], np.int32), candidates=np.stack([r[3] for r in res]))


# ---- the projection scene of tests/test_cpp_search.py and tests/test_search.py ------------------------------------------
PROJ_W, PROJ_CAP, PROJ_MARGIN = 4, 70, 8.0
IMG_W, IMG_H = L.IMG_W, L.IMG_H


def projection_scene():
    """Five old windows of PROJ_CAP slots and one predicted pose each: dict of olds (carry_ref windows, padded), news
    (their successors, for a carried PnP whose last poses are read in place), poses6 (5, 6) and what each window is
    there for:
    0  a pose inside the cloud and turned: landmarks in front of, behind and beside the camera,
       and slots that own no landmark (seen < 2) between them
    1  an angle beyond BA_MAX_THETA       2  a NaN in the pose
    3  an old window below the build's baseline gate: not ORBX_LM_OK
    4  an angle-axis vector on the small-angle branch"""
    rng = np.random.default_rng(2100)
    olds, news = [], []
    for w in range(5):
        st = CR.make_stream(2100 + w, 2 * PROJ_W - 1, 60)
        seen = rng.integers(1 if w == 0 else 0, PROJ_W + 1, 60)
        seen[:3] = PROJ_W, 0, 1
        old = CR.window(st, 0, PROJ_W, np.arange(60), seen)
        old = CR._pad_old(old, PROJ_CAP)
        if w == 3:
            old["poses"][1, 3:] = old["poses"][0, 3:] + np.array([0.01, 0.0, 0.02])
        olds.append(old)
        news.append(CR.successor(st, old, PROJ_W - 1, PROJ_W, [], cap=PROJ_CAP))
    poses6 = np.stack([o["true_poses"][-1] for o in olds])
    a = np.array([-0.2, 0.15, 0.5])
    poses6[0] = np.r_[a, -rodrigues(a) @ np.array([0.3, 0.0, 12.0])]
    poses6[1, :3] = np.array([0.0, 1.0, 0.0]) * 1.5e5
    poses6[2, 4] = np.nan
    poses6[4] = np.r_[np.array([3e-9, -8e-9, 5e-9]), [0.3, -0.1, -0.7]]
    return dict(olds=olds, news=news, poses6=poses6)


def check_projection_scene(block, ref):
    """Conditions on the REFERENCE: every window of the scene is what it is there for."""
    st, cnt = ref["state"], ref["count"]
    assert list(block["status"] == L.OK) == [True, True, True, False, True]
    assert all((st[0] == s).sum() >= 5 for s in (PROJ_NONE, PROJ_BEHIND, PROJ_OUTSIDE, PROJ_OK)), np.bincount(st[0])
    ok0 = np.flatnonzero(st[0] == PROJ_OK)
    assert (st[0][ok0[0]:ok0[-1]] == PROJ_NONE).any()  # NONE slots between the projected ones
    for w in (1, 2, 3):
        assert cnt[w] == 0 and not st[w].any() and not ref["xy"][w].any() and not ref["depth"][w].any()
    assert cnt[4] >= 20 and cnt[0] == (st[0] == PROJ_OK).sum()
    assert not ref["xy"][st != PROJ_OK].any() and not ref["depth"][st != PROJ_OK].any()


# ---- the gated sets ---------------------------------------------------------------------------------------------------
def gated_windows(qcap, tcap, frame, seed):
    """Four windows of described sets with positions in a frame (w, h): dict of qdesc, qstate, qxy (float32), tdesc,
    tstate, txy (float64), tpstate.  Queries are bit-flipped copies of train slots placed within a few pixels of them,
    with random ones among them; some slots of both sides are not OK, some positions are not finite, some predictions
    lie outside the frame and at 1e7.
    0  train positions spread over the frame           1  every train slot but a few inside one cell-sized clump
    2  no positioned train slot (every pstate BEHIND)  3  as window 0; the tests pass it with pstate left out"""
    rng = np.random.default_rng(seed)
    fw, fh = frame
    n = 4
    tdesc = rng.integers(0, 256, (n, tcap, 32), dtype=np.uint8)
    qdesc = rng.integers(0, 256, (n, qcap, 32), dtype=np.uint8)
    tstate = np.full((n, tcap), PD_OK, np.int32)
    qstate = np.full((n, qcap), PD_OK, np.int32)
    tpstate = np.full((n, tcap), PROJ_OK, np.int32)
    txy = np.stack([rng.uniform(0, fw - 1, (n, tcap)), rng.uniform(0, fh - 1, (n, tcap))], axis=-1)
    txy[1] = np.array([fw * 0.4, fh * 0.5]) + rng.uniform(-2.0, 2.0, (tcap, 2))  # a clump: hundreds of slots in one cell
    txy[1, :8] = np.stack([rng.uniform(0, fw - 1, 8), rng.uniform(0, fh - 1, 8)], axis=-1)
    qxy = np.stack([rng.uniform(0, fw - 1, (n, qcap)), rng.uniform(0, fh - 1, (n, qcap))], axis=-1).astype(np.float32)
    for w in range(n):
        for q in range(qcap):
            if q % 4 == 3:
                continue  # a random query at a random place
            t = int(rng.integers(0, tcap))
            qdesc[w, q] = R.flip(tdesc[w, t], rng, int(rng.integers(0, 50)))
            qxy[w, q] = (txy[w, t] + rng.uniform(-6.0, 6.0, 2)).astype(np.float32)
        # twins: train slots that share a descriptor at different places (d1 == d2 without the gate)
        for t in range(10, min(tcap, 60), 10):
            tdesc[w, t + 1] = tdesc[w, t]
        if w != 1:  # (the clump keeps its slots)
            tstate[w, 3::17], tstate[w, 5::23] = R.PD_NONE, R.PD_BORDER
            tpstate[w, 4::13], tpstate[w, 6::31] = PROJ_OUTSIDE, PROJ_NONE
        qstate[w, 2::19], qstate[w, 7::29] = R.PD_NONE, R.PD_BORDER
        txy[w, 9::37] = (-25.0, fh + 30.0)      # predictions outside the frame
        txy[w, 12::41] = (1e7, -1e7)            # and far away
        txy[w, 14::43, 0] = np.nan
        txy[w, 15::47, 1] = np.inf
        qxy[w, 11::53, 0] = np.nan
        qxy[w, 13::59, 1] = -np.inf
        qxy[w, 16::61] = (-12.5, fh + 4.25)     # a query outside the frame, near the outside predictions
    tpstate[2] = PROJ_BEHIND
    return dict(qdesc=qdesc, qstate=qstate, qxy=qxy, tdesc=tdesc, tstate=tstate, txy=txy, tpstate=tpstate)


def repeated_structure(n_pairs=40, seed=5):
    """One window in which every train descriptor appears twice, at two slots whose predictions lie 1100 pixels apart
    (slots p and n_pairs + p), each with a decoy of random bytes 5 pixels below it (slots 2 n_pairs + p and
    3 n_pairs + p); the pairs are 25 pixels apart along x.  Query q is a copy of pair q with q % 7 bits flipped, 3
    pixels right of the FIRST (even q) or the SECOND (odd q) of the two: at radius 10 its gate holds that slot and its
    decoy, and nothing else.  Returns the sets and the slot every query belongs to."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (n_pairs, 32), dtype=np.uint8)
    decoy = rng.integers(0, 256, (2 * n_pairs, 32), dtype=np.uint8)
    tdesc = np.concatenate([base, base, decoy])
    at = np.stack([50 + 25.0 * np.arange(n_pairs), rng.uniform(30, 340, n_pairs)], axis=-1)
    twice = np.concatenate([at, at + np.array([1100.0, 0.0])])
    txy = np.concatenate([twice, twice + np.array([0.0, 5.0])])
    right = np.array([q + n_pairs * (q % 2) for q in range(n_pairs)], np.int32)
    qdesc = np.stack([R.flip(base[q], rng, q % 7) for q in range(n_pairs)])
    qxy = (txy[right] + np.array([3.0, 0.0])).astype(np.float32)
    return dict(qdesc=qdesc[None], qstate=np.full((1, n_pairs), PD_OK, np.int32), qxy=qxy[None], tdesc=tdesc[None],
                tstate=np.full((1, 4 * n_pairs), PD_OK, np.int32), txy=txy[None], right=right)
