"""The forward-backward check of Lucas-Kanade over frame windows (DESIGN.md §9 rank 13;
orbx_lk_track_windows_fb_device and its companions): the HIP path against the restatement on the CPU oracle
(tests/lk_fb_ref.py), against the restatement driven by the GPU pair tracker, and against the plain windows call.
Positions, errors and distances are compared as uint32 bit patterns, `seen` and `lost` exactly, whole arrays including
the zero tail.  The shapes are those of tests/test_lk_windows.py."""
import numpy as np
import pytest

import lk_fb_ref as F
import lk_window_ref as R
from test_lk_oracle import smooth_image

pytestmark = pytest.mark.gpu
H, W = 96, 128
FIRST = [0, 3, 2, 3]
COUNTS = [300, 0, 7, 65]
K = np.array([[100.0, 0.0, 64.0], [0.0, 100.0, 48.0], [0.0, 0.0, 1.0]])


@pytest.fixture(scope="module")
def ctx(pkg):
    with pkg.Context(pkg.default_params("gpu", max_width=1241, max_height=376, max_batch=8)) as c:
        yield c


@pytest.fixture(scope="module")
def seq1():
    """8 frames of the seed-1 sequence and the 300 points, padded to 301 slots for each of 4 windows"""
    frames = R.shifted_frames(1, H, W, 8, (-2.4, 1.7))
    pts = np.zeros((4, 301, 2), np.float32)
    pts[:, :300] = R.box_points(1, 300, H, W)
    return frames, pts


@pytest.fixture(scope="module")
def ragged_ref(seq1):
    frames, pts = seq1
    ref = F.track_windows(frames, FIRST, 5, pts, 0.5, COUNTS, **R.REFERENCE)
    # conditions on the reference alone: every reason and every length in window 0, an empty window, two ragged ones
    assert [F.reasons(ref[4][w]) for w in range(4)] == [[83, 128, 2, 88], [301, 0, 0, 0], [297, 3, 0, 1],
                                                        [253, 23, 0, 25]]
    assert [R.lengths(ref[1][w], 5) for w in range(4)] == [[191, 13, 8, 6, 82], [0] * 5, [4, 0, 0, 0, 3],
                                                          [45, 2, 1, 0, 17]]
    for a in ref:
        a.setflags(write=False)
    return ref


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, ref):
    """(tracks, seen, err, fb_d2, lost) against (tracks, seen, err, fb_d2, lost)"""
    (gt, gs, ge, gd, gl), (rt, rs, re, rd, rl) = got, ref
    n = gt.shape[-2]
    assert gs.shape == rs.shape and np.array_equal(gs, rs), (R.lengths(gs, n), R.lengths(rs, n))
    assert gl.shape == rl.shape and np.array_equal(gl, rl), (F.reasons(gl), F.reasons(rl))
    assert gt.shape == rt.shape and np.array_equal(bits(gt), bits(rt))
    assert ge.shape == re.shape and np.array_equal(bits(ge), bits(re))
    assert gd.shape == rd.shape and np.array_equal(bits(gd), bits(rd))


def fetch(ctx, first=0, n=None):
    return ctx.lk_windows_fetch(first, n) + ctx.lk_windows_fb_fetch(first, n)


def gpu_pairs(ctx):
    return lambda prev, nxt, pts, **kw: ctx.lk_track(prev, nxt, pts, **kw)


def prefix_of_plain(fb, plain):
    """every slot's fb result is a prefix of the plain tracker's"""
    (tracks, seen, err), (pt, ps, pe) = fb[:3], plain
    assert (seen <= ps).all()
    k = np.arange(tracks.shape[-2])
    m = k < seen[..., None]
    assert np.array_equal(bits(tracks)[m], bits(pt)[m])
    assert np.array_equal(bits(err)[m[..., 1:]], bits(pe)[m[..., 1:]])


def test_one_window_against_the_restatement_and_the_pair_tracker(ctx):
    frames = R.shifted_frames(2, H, W, 5, (-6.5, 4.0))
    pts = R.box_points(2, 300, H, W)
    ref = F.track_window(frames, pts, 1.0, **R.REFERENCE)
    assert F.reasons(ref[4]) == [57, 158, 8, 77] and R.lengths(ref[1], 5) == [217, 9, 9, 8, 57]
    ctx.lk_track_windows(frames, [0], 5, pts[None], fb_threshold=1.0)
    got = [a[0] for a in fetch(ctx)]
    same(got, ref)
    same(got, F.track_window(frames, pts, 1.0, track=gpu_pairs(ctx), **R.REFERENCE))
    same(ctx.lk_track_window(frames, pts, fb_threshold=1.0), ref)  # the host entry


def test_ragged_batch_with_overlapping_windows(ctx, seq1, ragged_ref):
    """an empty window, partly filled workgroups, an odd slot stride; windows 1 and 3 share their frames"""
    import torch

    frames, pts = seq1
    t = torch.from_numpy(frames).cuda()
    ctx.lk_track_windows(t, FIRST, 5, pts, np.int32(COUNTS), fb_threshold=0.5)
    same(fetch(ctx), ragged_ref)
    same(fetch(ctx, 2, 1), [a[2:3] for a in ragged_ref])
    # window 3 in a batch of its own, every slot a point (d_counts = NULL)
    ctx.lk_track_windows(t, [3], 5, pts[3:4, :65].copy(), fb_threshold=0.5)
    same(fetch(ctx), [a[3:4, :65] for a in ragged_ref])
    # a count above the capacity is clamped
    ctx.lk_track_windows(t, [3], 5, pts[3:4, :65].copy(), np.int32([1000]), fb_threshold=0.5)
    same(fetch(ctx), [a[3:4, :65] for a in ragged_ref])
    try:
        ctx.lk_workspace_limit(1)  # one window is always granted: four slices
        ctx.lk_track_windows(t, FIRST, 5, pts, np.int32(COUNTS), fb_threshold=0.5)
        same(fetch(ctx), ragged_ref)
        ctx.lk_workspace_limit(6 * 6 * H * W)  # six frames: windows 0 | 1, 2, 3
        ctx.lk_track_windows(t, FIRST, 5, pts, np.int32(COUNTS), fb_threshold=0.5)
        same(fetch(ctx), ragged_ref)
    finally:
        ctx.lk_workspace_limit(0)  # the default again
    ctx.lk_track_windows(t, FIRST, 5, pts, np.int32(COUNTS), fb_threshold=0.5)
    same(fetch(ctx), ragged_ref)


def test_every_slot_is_a_prefix_of_the_plain_result(ctx, seq1, ragged_ref):
    frames, pts = seq1
    ctx.lk_track_windows(frames, FIRST, 5, pts, np.int32(COUNTS), fb_threshold=0.5)
    fb = fetch(ctx)
    ctx.lk_track_windows(frames, FIRST, 5, pts, np.int32(COUNTS))
    plain = ctx.lk_windows_fetch()
    prefix_of_plain(fb, plain)
    assert (fb[1] < plain[1]).sum() > 50  # the check ends tracks the plain tracker keeps
    # threshold +inf: only the two status tests are left; threshold 0: nothing returns exactly on moving frames
    ctx.lk_track_windows(frames, FIRST, 5, pts, np.int32(COUNTS), fb_threshold=np.inf)
    loose = fetch(ctx)
    same(loose, F.track_windows(frames, FIRST, 5, pts, np.inf, COUNTS, **R.REFERENCE))
    prefix_of_plain(loose, plain)
    assert not (loose[4] == 3).any() and (loose[4] == 2).any()
    ctx.lk_track_windows(frames, FIRST, 5, pts, np.int32(COUNTS), fb_threshold=0.0)
    same(fetch(ctx), F.track_windows(frames, FIRST, 5, pts, 0.0, COUNTS, **R.REFERENCE))


@pytest.fixture(scope="module")
def sweep_frames():
    f = smooth_image(5, 150, 211)
    return np.stack([f(0, 0), f(-2.4, 1.7), f(-4.8, 3.4)])


@pytest.mark.parametrize("win,max_level,max_iters,eps", [(21, 3, 30, 0.01), (5, 0, 10, 0.03), (31, 5, 3, 0.001),
                                                        (15, 7, 0, 0.01), (3, 1, 30, 0.01)])
def test_parameter_sweep_with_border_points(ctx, sweep_frames, win, max_level, max_iters, eps):
    rng = np.random.default_rng(win)
    pts = np.concatenate([
        np.stack([rng.uniform(-30, 240, 300), rng.uniform(-30, 180, 300)], 1),
        np.float32([[0, 0], [210, 149], [0.5, 148.5], [105.25, 74.75], [-21, 10], [211, 75], [1e4, 1e4], [-1e4, 3],
                    [np.nan, 5], [7, np.nan], [np.nan, np.nan]]),
    ]).astype(np.float32)
    kw = dict(win=win, max_level=max_level, max_iters=max_iters, epsilon=eps)
    ref = F.track_window(sweep_frames, pts, 0.5, **kw)
    assert (ref[1] == 3).sum() > 20 and (ref[4][-3:] == 1).all()
    ctx.lk_track_windows(sweep_frames, [0], 3, pts[None], fb_threshold=0.5, **kw)
    same([a[0] for a in fetch(ctx)], ref)


def test_flat_window_and_smallest_frame(ctx):
    pts = R.box_points(3, 100, 97, 131)
    flat = np.full((3, 97, 131), 200, np.uint8)
    ctx.lk_track_windows(flat, [0], 3, pts[None], fb_threshold=1.0)
    tracks, seen, err, d2, lost = fetch(ctx)
    assert (seen == 1).all() and (lost == 1).all()
    assert np.array_equal(bits(tracks[0, :, 0]), bits(pts)) and not tracks[0, :, 1:].any()
    assert not err.any() and not d2.any()
    f = smooth_image(46, 23, 23)
    small = np.stack([f(0, 0), f(-1.5, 0.75), f(-3.0, 1.5)])
    pts = R.box_points(4, 150, 23, 23)
    ref = F.track_window(small, pts, 1.0, **R.REFERENCE)
    assert (ref[1] > 1).sum() > 10
    ctx.lk_track_windows(small, [0], 3, pts[None], fb_threshold=1.0)
    same([a[0] for a in fetch(ctx)], ref)
    same(ctx.lk_track_window(small, pts, fb_threshold=1.0), ref)


def test_views_and_refusals(pkg, ctx, seq1, ragged_ref):
    frames, pts = seq1
    counts = np.int32(COUNTS)
    ctx.lk_track_windows(frames, FIRST, 5, pts, counts, fb_threshold=0.5)
    v, fv = ctx.lk_windows_view(), ctx.lk_windows_fb_view()
    assert (v.n_windows, v.slot_capacity, v.window_len) == (4, 301, 5)
    assert (fv.n_windows, fv.slot_capacity, fv.window_len) == (4, 301, 5)
    assert v.tracks_xy and v.seen and v.err and fv.fb_d2 and fv.lost
    assert fv.lost - fv.fb_d2 >= 4 * 4 * 301 * 4  # lost lies behind fb_d2 in the buffer of their own ...
    assert not (v.tracks_xy <= fv.fb_d2 < v.err + 4 * 4 * 301 * 4)  # ... which is not the result block
    # a bad threshold is refused and leaves the previous result
    for thr in (np.nan, -1.0, -np.inf):
        with pytest.raises(pkg.OrbxError) as e:
            ctx.lk_track_windows(frames, FIRST, 5, pts, counts, fb_threshold=thr)
        assert e.value.status == pkg.orbx.ERR_INVALID_ARG, thr
        with pytest.raises(pkg.OrbxError) as e:
            ctx.lk_track_window(frames[:3], pts[0], fb_threshold=thr)
        assert e.value.status == pkg.orbx.ERR_INVALID_ARG, thr
        same(fetch(ctx), ragged_ref)
    # so does every refusal of the plain entry
    for kw in (dict(window_first=[0, 4, 2, 3]), dict(window_len=1), dict(win=33), dict(max_level=8)):
        a = dict(window_first=FIRST, window_len=5)
        a.update(kw)
        with pytest.raises(pkg.OrbxError) as e:
            ctx.lk_track_windows(frames, a.pop("window_first"), a.pop("window_len"), pts, counts, fb_threshold=0.5, **a)
        assert e.value.status == pkg.orbx.ERR_INVALID_ARG, kw
        same(fetch(ctx), ragged_ref)
    with pytest.raises(pkg.OrbxError):
        ctx.lk_windows_fb_fetch(3, 2)
    # after a plain call the check's view and fetch are refused, the plain ones are not
    ctx.lk_track_windows(frames, FIRST, 5, pts, counts)
    for f in (ctx.lk_windows_fb_view, ctx.lk_windows_fb_fetch):
        with pytest.raises(pkg.OrbxError) as e:
            f()
        assert e.value.status == pkg.orbx.ERR_INVALID_ARG and "forward-backward" in str(e.value)
    assert ctx.lk_windows_view().n_windows == 4
    ctx.lk_track_windows(frames, FIRST, 5, pts, counts, fb_threshold=0.5)
    same(fetch(ctx), ragged_ref)


def test_fb_fetch_before_any_windows_call_is_refused(pkg):
    with pkg.Context(pkg.default_params("gpu", max_width=W, max_height=H, max_batch=2)) as c:
        with pytest.raises(pkg.OrbxError):
            c.lk_windows_fb_view()
        with pytest.raises(pkg.OrbxError):
            c.lk_windows_fb_fetch()


def flat(x):
    if isinstance(x, dict):
        return [(k, flat(x[k])) for k in sorted(x)]
    if isinstance(x, (list, tuple)):
        return [flat(a) for a in x]
    return (str(x.dtype), x.shape, x.tobytes())


def test_downstream_consumers_read_the_view_unchanged(ctx, seq1, ragged_ref):
    """the top-up (seeds = the last column, seen_min = window_len) and the tracks pose on the view of an fb call, and
    on device copies of the fetched arrays: bit-equal; the carried seeds are the slots the check left alive"""
    import torch

    frames, pts = seq1
    L, cap = 5, 301
    t = torch.from_numpy(frames).cuda()
    last = t[[f0 + L - 1 for f0 in FIRST]].contiguous()  # every window's last frame
    torch.cuda.synchronize()

    def consumers(tracks, seen):
        ctx.good_features_topup(last, tracks + 8 * (L - 1), seen, L, seed_capacity=cap, seed_point_stride=2 * L,
                                seed_frame_stride=2 * L * cap, max_corners=cap, quality_level=0.01, min_distance=8.0)
        ctx.tracks_pose(K, tracks, seen, 4, cap, L, max_iters=50)
        return (ctx.good_features_topup_fetch(), ctx.tracks_pose_fetch(),
                [ctx.tracks_pose_pair_fetch(p) for p in range(ctx.tracks_pose_view().n_pairs)])

    ctx.lk_track_windows(t, FIRST, L, pts, np.int32(COUNTS), fb_threshold=0.5)
    v = ctx.lk_windows_view()
    on_view = consumers(v.tracks_xy, v.seen)
    tracks, seen, err, d2, lost = fetch(ctx)
    same((tracks, seen, err, d2, lost), ragged_ref)
    d_tracks, d_seen = torch.from_numpy(tracks).cuda(), torch.from_numpy(seen).cuda()
    torch.cuda.synchronize()
    on_copies = consumers(d_tracks.data_ptr(), d_seen.data_ptr())
    assert flat(on_view) == flat(on_copies)
    counts, carried, points, origin = on_view[0]
    end = tracks[:, :, L - 1]
    inside = (end[..., 0] >= 0) & (end[..., 0] <= W - 1) & (end[..., 1] >= 0) & (end[..., 1] <= H - 1)
    alive = (lost == 0) & (seen > 0)
    assert np.array_equal(alive, seen == L)
    assert alive.sum(1).tolist() == [82, 0, 3, 17] and (alive & inside).sum(1).tolist() == [80, 0, 3, 16]
    for w in range(4):
        slots = np.flatnonzero(alive[w] & inside[w])  # (the top-up drops a seed that lies outside the frame)
        assert carried[w] == len(slots) and np.array_equal(origin[w, :carried[w]], slots)
        assert np.array_equal(bits(points[w, :carried[w]]), bits(end[w, slots]))
    # pair k of a window lists the slots with seen >= k + 2
    assert on_view[1]["n"].tolist() == [int((seen[w] >= k + 2).sum()) for w in range(4) for k in range(L - 1)]
