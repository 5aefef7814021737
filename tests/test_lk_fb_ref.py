"""The restatement of the forward-backward check (tests/lk_fb_ref.py) pinned on the CPU oracle
alone: conditions on the window every GPU test of the check uses, the subset property against the plain window
restatement (tests/lk_window_ref.py), and the edges of the threshold."""
import numpy as np
import pytest

import lk_fb_ref as F
import lk_window_ref as R

H, W, N = 96, 128, 5


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def window():
    frames = R.shifted_frames(2, H, W, N, (-6.5, 4.0))
    pts = R.box_points(2, 300, H, W)
    frames.setflags(write=False)
    pts.setflags(write=False)
    return frames, pts


@pytest.fixture(scope="module")
def plain(window):
    return R.track_window(*window, **R.REFERENCE)


@pytest.fixture(scope="module")
def fb1(window):
    return F.track_window(*window, 1.0, **R.REFERENCE)


def check_layout(res, n):
    """rule 5: what lies past `seen` is zero, what lies before it is set"""
    tracks, seen, err, d2, lost = res
    k = np.arange(n)[None]
    assert not tracks[k >= seen[:, None]].any() and not err[k[:, 1:] >= seen[:, None]].any()
    assert not d2[k[:, 1:] >= seen[:, None]].any()
    assert set(np.unique(lost)) <= {0, 1, 2, 3}
    assert np.array_equal(lost == 0, (seen == n) | (seen == 0))


def check_subset(res, plain_res):
    tracks, seen, err = res[:3]
    pt, ps, pe = plain_res
    assert (seen <= ps).all()
    k = np.arange(tracks.shape[1])[None]
    m = k < seen[:, None]
    assert np.array_equal(bits(tracks)[m], bits(pt)[m])
    assert np.array_equal(bits(err)[m[:, 1:]], bits(pe)[m[:, 1:]])


def test_conditions_on_the_reference(fb1):
    tracks, seen, err, d2, lost = fb1
    assert F.reasons(lost) == [57, 158, 8, 77]  # alive / forward / backward / over the threshold
    assert R.lengths(seen, N) == [217, 9, 9, 8, 57]
    assert min(F.reasons(lost)) >= 5 and (seen == N).sum() >= 30
    check_layout(fb1, N)
    # every pair that passed has a distance within the threshold, and some are not zero
    k = np.arange(1, N)[None]
    assert (d2[k < seen[:, None]] <= 1.0).all() and (d2 > 0).sum() > 100


def test_subset_of_the_plain_tracker(fb1, plain):
    check_subset(fb1, plain)
    assert (fb1[1] < plain[1]).sum() >= 50  # the check ends tracks the plain tracker keeps


def test_threshold_infinity_leaves_the_two_status_tests(window, plain):
    res = F.track_window(*window, np.inf, **R.REFERENCE)
    tracks, seen, err, d2, lost = res
    check_layout(res, N)
    check_subset(res, plain)
    ps = plain[1]
    assert F.reasons(lost) == [112, 177, 11, 0]
    # a forward loss is the plain tracker's loss, in the same pair; a backward loss comes in a pair the plain
    # tracker got through; and the plain tracker's losses not preceded by a backward loss are all forward losses
    assert np.array_equal(seen[lost == 1], ps[lost == 1]) and (ps[lost == 1] < N).all()
    assert (ps[lost == 2] > seen[lost == 2]).all()
    assert np.array_equal(lost == 1, (ps < N) & (lost != 2))
    assert (ps[lost == 0] == N).all()


def test_threshold_zero_passes_exact_returns_only(window, fb1):
    frames, pts = window
    res = F.track_window(frames, pts, 0.0, **R.REFERENCE)
    check_layout(res, N)
    # moving frames: no point returns exactly, so nothing gets past its first frame, and the reason is the one the
    # pair would have had anyway, or the distance
    assert (res[1] == 1).all() and not res[3].any() and F.reasons(res[4]) == [0, 149, 8, 143]
    # three times the same frame: every pass finds a zero mismatch and stays where it started, up to the rounding of
    # (x - half) + half.  Where that is exact, d2 == 0 passes; an ulp is already too far
    still = np.stack([frames[0]] * 3)
    res = F.track_window(still, pts, 0.0, **R.REFERENCE)
    loose = F.track_window(still, pts, np.inf, **R.REFERENCE)
    check_layout(res, 3)
    check_subset(res, loose[:3])
    passed = (np.arange(1, 3)[None] < loose[1][:, None]) & (loose[3] == 0)
    assert np.array_equal(res[1], 1 + np.cumprod(passed, 1).sum(1))
    assert not res[3].any() and (res[1] == 3).sum() > 50 and (res[4] == 3).sum() > 10


def test_no_iterations_return_the_point(window):
    """max_iters = 0: both passes return their start point, so r == p and d2 == 0 in every pair; the distance never
    fails.  A backward loss is then the minimum-eigenvalue or bounds test of frame k's own template at q == p (the
    forward pass ran them on frame k - 1's), which two slots of this window meet."""
    kw = dict(R.REFERENCE, max_iters=0)
    res = F.track_window(*window, 1.0, **kw)
    tracks, seen, err, d2, lost = res
    check_layout(res, N)
    check_subset(res, R.track_window(*window, **kw))
    assert not d2.any() and F.reasons(lost) == [159, 139, 2, 0]
    assert R.lengths(seen, N) == [141, 0, 0, 0, 159]
    live = seen == N
    assert np.array_equal(bits(tracks[live]), bits(np.repeat(window[1][live][:, None], N, 1)))


def test_counts_and_slots(window, fb1):
    frames, pts = window
    res = F.track_window(frames, pts, 1.0, count=7, slots=9, **R.REFERENCE)
    for a, b in zip(res, fb1):
        assert np.array_equal(a[:7].view(np.uint32), b[:7].view(np.uint32)) and not a[7:].any() and len(a) == 9
    batch = F.track_windows(frames, [0, 0], N, np.stack([pts, pts]), 1.0, counts=[300, 7], **R.REFERENCE)
    for a, b in zip(batch, fb1):
        assert np.array_equal(a[0].view(np.uint32), b.view(np.uint32))
        assert np.array_equal(a[1, :7].view(np.uint32), b[:7].view(np.uint32)) and not a[1, 7:].any()
