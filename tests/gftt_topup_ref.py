"""Numpy restatement of the masked Shi-Tomasi detection that tops up tracked points (rules
A-F): what orbx_good_features_topup_device, orbx_good_features_topup and orbx_good_features_to_track_masked compute,
bit for bit.  Independent of the kernels: whole-array numpy operations, the blocked pixels by brute force over every
(seed, pixel) pair -- no box, no bit map, no cell grid.  Rules 1-6 of rank 8 come from tests/gftt_ref.py."""
import numpy as np

import gftt_ref as G


def usable_seeds(seeds, w, h, seen=None, seen_min=0):
    """Rule A: the slots of the usable seeds, ascending.  seeds: (n, 2) float32; seen: (n,) int32 or None."""
    seeds = np.asarray(seeds, np.float32).reshape(-1, 2)
    x, y = seeds[:, 0], seeds[:, 1]
    live = np.ones(len(seeds), bool) if seen is None else np.asarray(seen, np.int32) >= seen_min
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(x) & np.isfinite(y) & (x >= np.float32(0)) & (x <= np.float32(w - 1)) & \
            (y >= np.float32(0)) & (y <= np.float32(h - 1))
    return np.flatnonzero(live & ok)


def blocked_by_seeds(carried_xy, w, h, min_distance):
    """Rule C: the (h, w) bool map of blocked pixels; every float32 operation on its own."""
    out = np.zeros((h, w), bool)
    if min_distance < 1:
        return out
    d2 = np.float32(np.float64(min_distance) * np.float64(min_distance))
    X = np.arange(w, dtype=np.float32)
    Y = np.arange(h, dtype=np.float32)
    for sx, sy in np.asarray(carried_xy, np.float32).reshape(-1, 2):
        dx, dy = X - sx, Y - sy
        t = (dx * dx)[None, :] + (dy * dy)[:, None]
        assert t.dtype == np.float32
        out |= t < d2
    return out


def masked_max(eig, blocked):
    """Rule D: the largest response over the pixels that are not blocked (0 when there is none)."""
    free = eig[~blocked]
    return free.max() if free.size else np.float32(0)


def candidates(eig, quality_level, blocked):
    """Rules D, E and 4: (values, row-major indices) of the candidates in selection order."""
    h, w = eig.shape
    mx = masked_max(eig, blocked)
    if not mx > 0:
        return np.zeros(0, np.float32), np.zeros(0, np.int64)
    thr = np.float32(np.float64(mx) * np.float64(quality_level))
    t = np.where(eig > thr, eig, np.float32(0))
    q = np.pad(t, 1, mode="constant", constant_values=0)
    dil = np.max([q[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], axis=0)  # blocked neighbours too
    cand = (t != 0) & (t == dil) & ~blocked
    cand[0, :] = cand[-1, :] = False
    cand[:, 0] = cand[:, -1] = False
    idx = np.flatnonzero(cand.reshape(-1))
    val = t.reshape(-1)[idx]
    order = np.lexsort((idx, val))[::-1]
    return val[order], idx[order]


def _detect(img, blocked, limit, quality_level, min_distance):
    """new corners (k, 2) float32 in acceptance order; limit None: no limit.  Also the intermediate results."""
    eig = G.corner_min_eigen_val(img)
    val, idx = candidates(eig, quality_level, blocked)
    w = eig.shape[1]
    if limit is not None and limit <= 0:
        kept = np.zeros(0, np.int64)
    else:
        kept = G.select(idx, w, 0 if limit is None else limit, min_distance)
    k = idx[kept]
    new = np.stack([(k % w).astype(np.float32), (k // w).astype(np.float32)], axis=1).reshape(-1, 2)
    return new, dict(eig=eig, values=val, indices=idx, kept=kept, blocked=blocked)


def top_up(img, seeds, max_corners, quality_level, min_distance, seen=None, seen_min=0, full=False):
    """Rules A-F for one frame: (points (count, 2) float32, origin (count,) int32, carried)."""
    assert max_corners >= 1
    img = np.asarray(img)
    h, w = img.shape
    seeds = np.asarray(seeds, np.float32).reshape(-1, 2)
    slots = usable_seeds(seeds, w, h, seen, seen_min)[:max_corners]  # rule B
    carried = seeds[slots]
    blocked = blocked_by_seeds(carried, w, h, min_distance)
    new, info = _detect(img, blocked, max_corners - len(slots), quality_level, min_distance)
    points = np.concatenate([carried, new]).astype(np.float32).reshape(-1, 2)
    origin = np.concatenate([slots, np.full(len(new), -1)]).astype(np.int32)
    if full:
        return points, origin, len(slots), info
    return points, origin, len(slots)


def good_features_to_track_masked(img, mask, max_corners, quality_level, min_distance, full=False):
    """cv::goodFeaturesToTrack with a mask: a pixel is blocked iff its mask byte is 0; max_corners <= 0: no limit."""
    blocked = np.asarray(mask) == 0
    assert blocked.shape == np.asarray(img).shape
    new, info = _detect(img, blocked, max_corners if max_corners > 0 else None, quality_level, min_distance)
    return (new, info) if full else new


def batch_arrays(results, slot_capacity):
    """whole result arrays of a batch of top_up() results: counts, carried, points (n, cap, 2), origin (n, cap);
    slots at or beyond counts[f] are 0 with origin -1"""
    n = len(results)
    counts, carried = np.zeros(n, np.int32), np.zeros(n, np.int32)
    points = np.zeros((n, slot_capacity, 2), np.float32)
    origin = np.full((n, slot_capacity), -1, np.int32)
    for f, (p, o, c) in enumerate(r[:3] for r in results):
        counts[f], carried[f] = len(p), c
        points[f, :len(p)] = p
        origin[f, :len(p)] = o
    return counts, carried, points, origin
