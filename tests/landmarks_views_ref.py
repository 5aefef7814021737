"""Independent numpy restatement of the landmarks build from every view of a track with its reprojection gate
(rules 1-8; include/orbx_lm.h), beside tests/landmarks_ref.py, whose scenes and Rodrigues it
uses.

Nothing here shares code with the library: the DLT is numpy.linalg.svd of the 2 m x 4 system of the m views used (the
library diagonalises its 4 x 4 normal matrix with Jacobi sweeps), depth and reprojection are plain matrix products."""
import numpy as np

import landmarks_ref as R

FIRST_TWO, WIDEST, ALL_VIEWS = range(3)
KEPT, SHORT, DEGENERATE, BEHIND, REPROJECTION, NO_WINDOW = range(6)


def views_used(tri_mode, sn):
    return {FIRST_TWO: [0, 1], WIDEST: [0, sn - 1], ALL_VIEWS: list(range(sn))}[tri_mode]


def np_dlt_views(Ps, pix):
    """The homogeneous point of the views with projection matrices Ps and pixels pix."""
    A = []
    for P, (x, y) in zip(Ps, pix):
        A += [x * P[2] - P[0], y * P[2] - P[1]]
    return np.linalg.svd(np.array(A))[2][-1]


def np_build_views(K, poses, tracks, seen, tri_mode, max_reproj_px):
    """One window by rules 1-8: dict of status, reason (slots,), reproj_px (slots,) float64, max_e2 (slots,), min_depth
    (slots,: the depth the mode judges by -- world z for FIRST_TWO, else the smallest camera depth over the observed
    views --, nan where there is no point), points (N, 3) and
    slot_of_point (N,)."""
    poses = np.asarray(poses, float).reshape(-1, 6)
    W, slots = len(poses), len(seen)
    n_prep = 2 if tri_mode == FIRST_TWO and not max_reproj_px > 0 else W
    out = dict(status=R.OK, reason=np.full(slots, NO_WINDOW, np.uint8), reproj_px=np.zeros(slots),
               max_e2=np.zeros(slots), min_depth=np.full(slots, np.nan), points=np.zeros((0, 3)),
               slot_of_point=np.zeros(0, np.int32))
    if any(np.linalg.norm(p[:3]) > 1e5 for p in poses[:n_prep]):
        out["status"] = R.BAD_POSE
        return out
    b = float(np.linalg.norm(poses[0, 3:] - poses[1, 3:]))
    if b < 0.1 or b > 100.0:
        out["status"] = R.BASELINE
        return out
    Rt = [np.c_[R.rodrigues(p[:3]), p[3:]] for p in poses[:n_prep]]
    P = [K @ m for m in Rt]
    pts, slot = [], []
    for s in range(slots):
        sn = int(min(max(seen[s], 0), W))
        if sn < 2:
            out["reason"][s] = SHORT
            continue
        t = np.asarray(tracks[s], np.float64)
        used = views_used(tri_mode, sn)
        h = np_dlt_views([P[k] for k in used], [t[k] for k in used])
        with np.errstate(all="ignore"):
            X = h[:3] / h[3]
        if h[3] == 0.0 or not np.all(np.isfinite(X)):
            out["reason"][s] = DEGENERATE
            continue
        observed = range(min(sn, n_prep))
        Xh = np.r_[X, 1.0]
        depth = [float(Rt[k][2] @ Xh) for k in observed]
        out["min_depth"][s] = X[2] if tri_mode == FIRST_TWO else min(depth)
        behind = not X[2] > 0.0 if tri_mode == FIRST_TWO else any(not d > 0.0 for d in depth)
        e2 = []
        with np.errstate(all="ignore"):
            for k in observed:
                q = P[k] @ Xh
                e2.append(float((q[0] / q[2] - t[k, 0]) ** 2 + (q[1] / q[2] - t[k, 1]) ** 2))
        bad = not np.all(np.isfinite(e2))
        max_e2 = max([0.0] + [e for e in e2 if np.isfinite(e)])
        out["max_e2"][s] = max_e2
        out["reproj_px"][s] = np.inf if bad else np.sqrt(max_e2)
        if behind:
            out["reason"][s] = BEHIND
        elif max_reproj_px > 0 and (bad or max_e2 > max_reproj_px ** 2):
            out["reason"][s] = REPROJECTION
        else:
            out["reason"][s] = KEPT
            pts.append(X), slot.append(s)
    if not pts:
        out["status"] = R.EMPTY
        return out
    out["points"], out["slot_of_point"] = np.array(pts), np.array(slot, np.int32)
    return out
