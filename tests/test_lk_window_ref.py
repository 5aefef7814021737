"""The window restatement (tests/lk_window_ref.py) of trackPointsAcrossWindow (src/with_bundle_adjustment.cpp:464-499)
on a sequence with a known answer, and the conditions the GPU tests (tests/test_lk_windows.py) rely on, checked on the
oracle alone.  No GPU."""
import numpy as np

import lk_window_ref as R

H, W = 96, 128


def test_known_translation_through_five_frames():
    """Frame k is the texture shifted by k * (-2.4, 1.7), so its content moves by (+2.4, -1.7) per frame: a track that
    starts and ends at least 15 px inside the image and survives all 5 frames ends at start + 4 * (2.4, -1.7).
    The oracle gives 49 such tracks, median error 0.014 px, largest 0.056 px; the bounds are about 4x that."""
    frames = R.shifted_frames(1, H, W, 5, (-2.4, 1.7))
    pts = R.box_points(1, 300, H, W)
    tracks, seen, err = R.track_window(frames, pts, **R.REFERENCE)

    def inside(p):
        return (p[:, 0] >= 15) & (p[:, 0] <= W - 15) & (p[:, 1] >= 15) & (p[:, 1] <= H - 15)

    m = (seen == 5) & inside(tracks[:, 0]) & inside(tracks[:, 4])
    d = np.abs(tracks[m, 4] - tracks[m, 0] - 4 * np.float32([2.4, -1.7])).max(1)
    print("tracks %d median %.4f max %.4f" % (m.sum(), np.median(d), d.max()))
    assert m.sum() >= 40
    assert np.median(d) < 0.05
    assert d.max() < 0.25


def test_layout_and_zero_tail():
    frames = R.shifted_frames(2, H, W, 5, (-6.5, 4.0))
    pts = R.box_points(2, 300, H, W)
    tracks, seen, err = R.track_window(frames, pts, count=290, slots=303, **R.REFERENCE)
    assert tracks.shape == (303, 5, 2) and seen.shape == (303,) and err.shape == (303, 4)
    assert np.array_equal(tracks[:290, 0], pts[:290]) and seen[:290].min() >= 1 and seen.max() == 5
    assert not seen[290:].any() and not tracks[290:].any() and not err[290:].any()
    for i in range(290):
        assert not tracks[i, seen[i]:].any() and not err[i, max(seen[i] - 1, 0):].any()
    # every exit path: tracks of every length (the oracle gives 149 / 14 / 8 / 10 / 119 with all 300 points)
    full = R.track_window(frames, pts, **R.REFERENCE)[1]
    assert R.lengths(full, 5) == [149, 14, 8, 10, 119]
    # the survivors-only chain equals tracking every point on its own, as the reference does
    for i in (0, 17, 123, 299):
        t1, s1, e1 = R.track_window(frames, pts[i:i + 1], **R.REFERENCE)
        assert s1[0] == full[i]
