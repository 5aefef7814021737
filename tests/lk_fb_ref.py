"""The forward-backward check of the windows tracker restated on top of the LK oracle
(oracle_lib.lk_track), in the shape of lk_window_ref.track_window.  For the point p of a live slot entering pair k
(frames k - 1 -> k):

 1. forward   (q, st_f, e_f) = track(frame k - 1, frame k, p); st_f == 0 ends the track, reason 1
 2. backward  (r, st_b, .) = track(frame k, frame k - 1, q), started at q itself; st_b == 0 ends it, reason 2
 3. distance  dx = r.x - p.x, dy = r.y - p.y, one float32 subtraction each; d2 = dx * dx + dy * dy in binary64 (the
              products of two widened floats are exact, the sum is rounded once); the pair passes iff
              d2 <= float64(thr) * float64(thr) with thr a float32; a NaN d2 fails; failing ends it, reason 3
 4. on a pass tracks[k] = q, err[k - 1] = e_f, fb_d2[k - 1] = float32(d2), and q enters pair k + 1

Every pass of a pair is run on the slots still alive only.  Results: tracks (slots, n, 2), seen (slots,), err
(slots, n - 1) in the layout of orbx_lk_windows_view, fb_d2 (slots, n - 1) float32 and lost (slots,) int32, zero past
`seen` (fb_d2: past seen - 1 pairs) and in the slots at or beyond `count`; lost is 0 for a track alive through the
window."""
import numpy as np

import oracle_lib as O

ALIVE, FORWARD, BACKWARD, DISTANCE = range(4)


def distance2(r, p):
    """rule 3's d2 for rows of float32 points"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = (np.asarray(r, np.float32) - np.asarray(p, np.float32)).astype(np.float32).astype(np.float64)
        return d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]


def track_window(frames, pts, thr, count=None, slots=None, track=None, **kw):
    """frames: the window's images; pts: (n, 2) points of frames[0]; thr: the threshold (a float32 value, >= 0 or
    +inf); count, slots, track, kw as lk_window_ref.track_window.  Returns tracks, seen, err, fb_d2, lost."""
    track = track or O.lk_track
    thr = np.float32(thr)
    assert thr >= 0, "the entries refuse a NaN or negative threshold"
    with np.errstate(over="ignore"):
        thr2 = np.float64(thr) * np.float64(thr)
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    slots = len(pts) if slots is None else slots
    count = min(len(pts) if count is None else count, slots)
    n = len(frames)
    tracks = np.zeros((slots, n, 2), np.float32)
    seen = np.zeros(slots, np.int32)
    err = np.zeros((slots, n - 1), np.float32)
    fb_d2 = np.zeros((slots, n - 1), np.float32)
    lost = np.zeros(slots, np.int32)
    tracks[:count, 0] = pts[:count]
    seen[:count] = 1
    live = np.arange(count)
    cur = pts[:count].copy()
    for k in range(1, n):
        if len(live) == 0:
            break
        q, st, e = track(frames[k - 1], frames[k], cur, **kw)[:3]
        ok = st == 1
        lost[live[~ok]] = FORWARD
        live, cur, q, e = live[ok], cur[ok], q[ok], e[ok]
        if len(live) == 0:
            break
        r, st = track(frames[k], frames[k - 1], q, **kw)[:2]
        ok = st == 1
        lost[live[~ok]] = BACKWARD
        live, cur, q, e, r = live[ok], cur[ok], q[ok], e[ok], r[ok]
        d2 = distance2(r, cur)
        ok = d2 <= thr2  # (False for NaN)
        lost[live[~ok]] = DISTANCE
        live, cur, e, d2 = live[ok], q[ok], e[ok], d2[ok]
        tracks[live, k] = cur
        err[live, k - 1] = e
        with np.errstate(over="ignore"):
            fb_d2[live, k - 1] = d2.astype(np.float32)
        seen[live] = k + 1
    return tracks, seen, err, fb_d2, lost


def track_windows(frames, window_first, window_len, points, thr, counts=None, track=None, **kw):
    """The batch: points (n_windows, slots, 2), counts (n_windows,) or None.  Returns the five arrays with a leading
    window axis."""
    points = np.asarray(points, np.float32)
    res = [track_window([frames[f0 + k] for k in range(window_len)], points[w], thr,
                        None if counts is None else int(counts[w]), points.shape[1], track, **kw)
           for w, f0 in enumerate(window_first)]
    return tuple(np.stack([r[i] for r in res]) for i in range(5))


def reasons(lost):
    """slots per value of lost, 0 .. 3"""
    return [int((lost == k).sum()) for k in range(4)]
