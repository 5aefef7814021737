"""trackPointsAcrossWindow (src/with_bundle_adjustment.cpp:464-499) restated on top of the LK oracle
(oracle_lib.lk_track): the points of the window's first frame are followed pair by pair, every pair is tracked on
the SURVIVORS only, and a track ends with the first pair that loses it.  Results come in the layout of
orbx_lk_windows_view: tracks (slots, window_len, 2), seen (slots,), err (slots, window_len - 1), zero past `seen`
and in the slots at or beyond `count`."""
import numpy as np

import oracle_lib as O

REFERENCE = dict(win=21, max_level=3, max_iters=30, epsilon=0.01)  # with_bundle_adjustment.cpp:485-486


def track_window(frames, pts, count=None, slots=None, track=None, **kw):
    """frames: the window's images; pts: (n, 2) points of frames[0]; count: how many of them are used (None: all);
    slots: rows of the result (None: n).  track(prev, next, pts, **kw) -> (next_pts, status, err, ...) is the
    per-pair tracker, the oracle's by default."""
    track = track or O.lk_track
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    slots = len(pts) if slots is None else slots
    count = min(len(pts) if count is None else count, slots)
    n = len(frames)
    tracks = np.zeros((slots, n, 2), np.float32)
    seen = np.zeros(slots, np.int32)
    err = np.zeros((slots, n - 1), np.float32)
    tracks[:count, 0] = pts[:count]
    seen[:count] = 1
    live = np.arange(count)
    cur = pts[:count].copy()
    for k in range(1, n):
        if len(live) == 0:
            break
        out, st, e = track(frames[k - 1], frames[k], cur, **kw)[:3]
        ok = st == 1
        live, cur = live[ok], out[ok]
        tracks[live, k] = cur
        err[live, k - 1] = e[ok]
        seen[live] = k + 1
    return tracks, seen, err


def track_windows(frames, window_first, window_len, points, counts=None, track=None, **kw):
    """The batch: points (n_windows, slots, 2), counts (n_windows,) or None.  Returns the three arrays with a leading
    window axis."""
    points = np.asarray(points, np.float32)
    res = [track_window([frames[f0 + k] for k in range(window_len)], points[w],
                        None if counts is None else int(counts[w]), points.shape[1], track, **kw)
           for w, f0 in enumerate(window_first)]
    return tuple(np.stack([r[i] for r in res]) for i in range(3))


def lengths(seen, window_len):
    """tracks per length 1 .. window_len"""
    return [int((seen == k).sum()) for k in range(1, window_len + 1)]


def shifted_frames(seed, h, w, n, step):
    """n frames of tests/test_lk_oracle.py's smooth_image(seed, h, w), frame k shifted by k * step"""
    from test_lk_oracle import smooth_image

    f = smooth_image(seed, h, w)
    return np.stack([f(k * step[0], k * step[1]) for k in range(n)])


def box_points(seed, n, h, w):
    """n points uniform in [-30, w + 30] x [-30, h + 30]"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-30, w + 30, n), rng.uniform(-30, h + 30, n)], 1).astype(np.float32)
