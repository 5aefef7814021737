"""Lucas-Kanade over frame windows (orbx_lk_track_windows_device and its companions): the HIP
path against the window restatement on the CPU oracle (tests/lk_window_ref.py) and against chains of per-pair
orbx_lk_track calls.  Positions and errors are compared as uint32 bit patterns, `seen` exactly, whole arrays
including the zero tail."""
import numpy as np
import pytest

import lk_cases as K
import lk_ref
import lk_window_ref as R
import oracle_lib as O
from test_lk_oracle import smooth_image

pytestmark = pytest.mark.gpu
H, W = 96, 128
FIRST = [0, 3, 2, 3]
COUNTS = [300, 0, 7, 65]


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
    ref = R.track_windows(frames, FIRST, 5, pts, COUNTS, **R.REFERENCE)
    # conditions on the reference alone
    assert [R.lengths(ref[1][w], 5) for w in range(4)] == [[127, 0, 2, 5, 166], [0] * 5, [3, 0, 0, 0, 4],
                                                          [23, 2, 2, 0, 38]]
    for a in ref:
        a.setflags(write=False)
    return ref


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, ref):
    (gt, gs, ge), (rt, rs, re) = got, ref
    assert gs.shape == rs.shape and np.array_equal(gs, rs), (R.lengths(gs, gt.shape[-2]), R.lengths(rs, rt.shape[-2]))
    assert gt.shape == rt.shape and np.array_equal(bits(gt), bits(rt))
    assert ge.shape == re.shape and np.array_equal(bits(ge), bits(re))


def gpu_pairs(ctx):
    return lambda prev, nxt, pts, **kw: ctx.lk_track(prev, nxt, pts, **kw)


def test_tracks_end_in_every_frame(ctx):
    frames = R.shifted_frames(2, H, W, 5, (-6.5, 4.0))
    pts = R.box_points(2, 300, H, W)
    ref = R.track_window(frames, pts, **R.REFERENCE)
    assert min(R.lengths(ref[1], 5)) >= 5  # every exit path is taken
    ctx.lk_track_windows(frames, [0], 5, pts[None])
    got = ctx.lk_windows_fetch()
    same([a[0] for a in got], ref)
    same([a[0] for a in got], R.track_window(frames, pts, track=gpu_pairs(ctx), **R.REFERENCE))
    same(ctx.lk_track_window(frames, pts), ref)  # the host entry


def test_ragged_batch_with_overlapping_windows(ctx, seq1, ragged_ref):
    """an empty window, partly filled workgroups, an odd slot stride; windows 1 and 3 share their frames"""
    import torch

    frames, pts = seq1
    t = torch.from_numpy(frames).cuda()
    ctx.lk_track_windows(t, FIRST, 5, pts, np.int32(COUNTS))
    v = ctx.lk_windows_view()
    assert (v.n_windows, v.slot_capacity, v.window_len) == (4, 301, 5)
    same(ctx.lk_windows_fetch(), ragged_ref)
    same(ctx.lk_windows_fetch(2, 1), [a[2:3] for a in ragged_ref])
    # window 3 in a batch of its own, every slot a point (d_counts = NULL)
    ctx.lk_track_windows(t, [3], 5, pts[3:4, :65].copy())
    same(ctx.lk_windows_fetch(), [a[3:4, :65] for a in ragged_ref])
    # a count above the capacity is clamped
    ctx.lk_track_windows(t, [3], 5, pts[3:4, :65].copy(), np.int32([1000]))
    same(ctx.lk_windows_fetch(), [a[3:4, :65] for a in ragged_ref])


def test_windows_of_two_frames_are_the_per_pair_tracker(ctx, seq1):
    frames, pts = seq1
    p = np.repeat(pts[:1, :300], 7, 0)
    ctx.lk_track_windows(frames, np.arange(7), 2, p)
    tracks, seen, err = ctx.lk_windows_fetch()
    for k in range(7):
        out, st, e = ctx.lk_track(frames[k], frames[k + 1], p[k])
        ro, rs, re, _ = O.lk_track(frames[k], frames[k + 1], p[k])
        assert np.array_equal(st, rs) and np.array_equal(bits(out), bits(ro)) and np.array_equal(bits(e), bits(re))
        assert np.array_equal(seen[k], 1 + st.astype(np.int32)) and 0 < st.sum() < 300
        assert np.array_equal(bits(tracks[k, :, 1]), bits(np.where(st[:, None] == 1, out, 0)))
        assert np.array_equal(bits(err[k, :, 0]), bits(np.where(st == 1, e, 0)))
        assert np.array_equal(bits(tracks[k, :, 0]), bits(p[k]))


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
        np.float32([[0, 0], [210, 149], [0.5, 148.5], [105.25, 74.75], [-21, 10], [211, 75], [1e4, 1e4], [-1e4, 3]]),
    ]).astype(np.float32)
    kw = dict(win=win, max_level=max_level, max_iters=max_iters, epsilon=eps)
    ctx.lk_track_windows(sweep_frames, [0], 3, pts[None], **kw)
    same([a[0] for a in ctx.lk_windows_fetch()], R.track_window(sweep_frames, pts, **kw))


def test_flat_window_and_smallest_frame(ctx):
    pts = R.box_points(3, 100, 97, 131)
    flat = np.full((3, 97, 131), 200, np.uint8)
    ctx.lk_track_windows(flat, [0], 3, pts[None])
    tracks, seen, err = ctx.lk_windows_fetch()
    assert (seen == 1).all() and np.array_equal(bits(tracks[0, :, 0]), bits(pts)) and not tracks[0, :, 1:].any()
    assert not err.any()
    f = smooth_image(46, 23, 23)
    small = np.stack([f(0, 0), f(-1.5, 0.75), f(-3.0, 1.5)])
    pts = R.box_points(4, 150, 23, 23)
    ref = R.track_window(small, pts, **R.REFERENCE)
    assert (ref[1] > 1).sum() > 10
    ctx.lk_track_windows(small, [0], 3, pts[None])
    same([a[0] for a in ctx.lk_windows_fetch()], ref)
    same(ctx.lk_track_window(small, pts), ref)


def test_special_points_against_the_numpy_restatement(ctx):
    """Three overlapping windows of three 56 x 48 frames, 64 slots, ragged counts, the special points of
    tests/lk_cases.py (bounds from both sides, NaN, infinities, values beyond int32) among random ones: the chain of
    tests/lk_window_ref.py on the numpy tracker (tests/lk_ref.py) and on the oracle, bit for bit.  A NaN point is seen
    in its first frame only."""
    h, w = 48, 56
    frames = R.shifted_frames(7, h, w, 5, (-1.3, 0.6))
    special = K.special_points(21, w, h)
    rng = np.random.default_rng(56)
    pts = np.stack([rng.uniform(-12, w + 12, (3, 64)), rng.uniform(-12, h + 12, (3, 64))], 2).astype(np.float32)
    pts[0, :len(special)] = special
    pts[1, 2:5] = special[21:24]               # the NaN points inside a window of 5 points
    pts[2, 64 - len(special):] = special[::-1]
    first, counts = [0, 2, 1], np.int32([64, 5, 61])
    ref = R.track_windows(frames, first, 3, pts, counts, track=lk_ref.track, **R.REFERENCE)
    assert [R.lengths(ref[1][k], 3)[2] > 0 for k in range(3)] == [True] * 3  # tracks that live through each window
    ctx.lk_track_windows(frames, first, 3, pts, counts)
    got = ctx.lk_windows_fetch()
    same(got, ref)
    same(got, R.track_windows(frames, first, 3, pts, counts, **R.REFERENCE))
    tracks, seen, err = got
    nan = np.isnan(pts).any(2) & (np.arange(64)[None] < counts[:, None])
    assert nan.sum() == 3 + 3 + 3 and (seen[nan] == 1).all()
    assert np.array_equal(bits(tracks[nan][:, 0]), bits(pts[nan])) and not tracks[nan][:, 1:].any() and not err[nan].any()
    same(ctx.lk_track_window(frames[:3], pts[0]), [a[0] for a in ref])  # the host entry


def strided(frames, fill_seed):
    """the frames as a region of a larger device tensor: odd byte offset, row stride width + 13, random gaps"""
    import torch

    n, h, w = frames.shape
    base, rs = 3, w + 13
    fs = rs * h + 5
    buf = np.random.default_rng(fill_seed).integers(0, 256, base + n * fs, dtype=np.uint8)
    np.lib.stride_tricks.as_strided(buf[base:], shape=(n, h, w), strides=(fs, rs, 1))[...] = frames
    t = torch.from_numpy(buf).cuda()
    return torch.as_strided(t, (n, h, w), (fs, rs, 1), base)


def test_strided_frames_with_garbage_gaps(ctx, seq1, ragged_ref):
    frames, pts = seq1
    for fill_seed in (10, 11):
        ctx.lk_track_windows(strided(frames, fill_seed), FIRST, 5, pts, np.int32(COUNTS))
        same(ctx.lk_windows_fetch(), ragged_ref)


def test_workspace_limit_runs_slices_of_whole_windows(ctx, seq1, ragged_ref):
    frames, pts = seq1
    try:
        ctx.lk_workspace_limit(1)  # one window is always granted: four slices
        ctx.lk_track_windows(frames, FIRST, 5, pts, np.int32(COUNTS))
        same(ctx.lk_windows_fetch(), ragged_ref)
        ctx.lk_workspace_limit(6 * 6 * H * W)  # six frames: windows 0 | 1, 2, 3
        ctx.lk_track_windows(frames, FIRST, 5, pts, np.int32(COUNTS))
        same(ctx.lk_windows_fetch(), ragged_ref)
    finally:
        ctx.lk_workspace_limit(0)  # the default again
    ctx.lk_track_windows(frames, FIRST, 5, pts, np.int32(COUNTS))
    same(ctx.lk_windows_fetch(), ragged_ref)


def test_other_results_and_the_per_pair_state_are_untouched(ctx, seq1, ragged_ref):
    import torch

    kitti = O.load_kitti(0)
    crops = np.stack([np.ascontiguousarray(kitti[100 + 2 * i:260 + 2 * i, 300 + 3 * i:620 + 3 * i]) for i in range(3)])
    t = torch.from_numpy(crops).cuda()
    torch.cuda.synchronize()
    cap = ctx.plan(320, 160)["out_capacity"]
    frames, pts = seq1
    a, b, c3 = frames[0], frames[1], frames[2]
    p = pts[0, :300]

    def snapshot():
        out = [ctx.batch_fetch(0, 3, cap)]
        out += [ctx.batch_match_fetch(pair, cap) for pair in (0, 1)]
        return out, ctx.good_features_fetch()

    ctx.batch_device(t.data_ptr(), 3, 320, 160)
    ctx.batch_match_consecutive(0.8)
    ctx.good_features_batch(t, 500, 0.01, 8.0)
    ctx.lk_track(a, b, p)
    before, gf_before = snapshot()
    assert before[0]["counts"].min() > 50 and len(before[1][0]) > 10 and len(gf_before[0]) > 50
    ctx.lk_track_windows(frames, FIRST, 5, pts, np.int32(COUNTS))
    same(ctx.lk_windows_fetch(), ragged_ref)
    after, gf_after = snapshot()
    for k in before[0]:
        assert np.array_equal(before[0][k], after[0][k]), k
    for pair in (1, 2):
        assert all(np.array_equal(x, y) for x, y in zip(before[pair], after[pair]))
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(gf_before, gf_after))
    # prev == NULL still continues from b
    go, gs, ge = ctx.lk_track(None, c3, p)
    ro, rs, re, _ = O.lk_track(b, c3, p)
    assert np.array_equal(gs, rs) and np.array_equal(bits(go), bits(ro)) and np.array_equal(bits(ge), bits(re))
    same(ctx.lk_windows_fetch(), ragged_ref)  # and the windows result outlives the per-pair call


def test_callers_stream_may_be_destroyed_after_the_call(pkg, ctx, seq1, ragged_ref):
    import ctypes as C

    import torch

    frames, pts = seq1
    t = torch.from_numpy(frames).cuda()
    d_pts = torch.from_numpy(pts).cuda()
    d_counts = torch.from_numpy(np.int32(COUNTS)).cuda()
    torch.cuda.synchronize()
    hip = pkg.orbx.load()  # (the HIP runtime liborbx.so is linked to: a stream of the caller's own)
    s = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s)) == 0
    ctx.lk_track_windows(t, FIRST, 5, d_pts, d_counts, stream=s.value)
    assert hip.hipStreamDestroy(s) == 0
    same(ctx.lk_windows_fetch(), ragged_ref)
    ctx.lk_track_windows(t, FIRST, 5, d_pts, d_counts)  # the next call, on the context's stream
    same(ctx.lk_windows_fetch(), ragged_ref)


def test_device_chain_from_good_features(ctx):
    """the good-features view's corners_xy / counts handed straight to the tracker: nothing visits the host"""
    import torch

    crops = np.stack([np.ascontiguousarray(O.load_kitti(i)[100:260, 300:620]) for i in (0, 1)])
    t = torch.from_numpy(crops).cuda()
    torch.cuda.synchronize()
    ctx.good_features_batch(t, 2000, 0.01, 8.0)
    v = ctx.good_features_view()
    ctx.lk_track_windows(t, [0], 2, v.corners_xy, v.counts, slot_capacity=v.slot_capacity)
    got = ctx.lk_windows_fetch()
    corners = ctx.good_features_fetch()[0]
    assert 100 < len(corners) <= v.slot_capacity
    ref = R.track_window(crops, corners, slots=v.slot_capacity, **R.REFERENCE)
    assert (ref[1][:len(corners)] == 2).mean() > 0.9
    same([a[0] for a in got], ref)


def test_device_chain_from_good_features_across_callers_streams(pkg, ctx):
    """the same chain with the corners made on one caller's stream and tracked on another, and no host synchronisation
    in between: the tracker's stream has to wait for the good-features event before it reads the view"""
    import ctypes as C

    import torch

    crops = np.stack([np.ascontiguousarray(O.load_kitti(i)[100:260, 300:620]) for i in (0, 1)])
    t = torch.from_numpy(crops).cuda()
    torch.cuda.synchronize()
    hip = pkg.orbx.load()
    sa, sb = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(sa)) == 0 and hip.hipStreamCreate(C.byref(sb)) == 0
    ctx.good_features_batch(t, 2000, 0.01, 8.0, stream=sa.value)
    v = ctx.good_features_view()
    ctx.lk_track_windows(t, [0], 2, v.corners_xy, v.counts, slot_capacity=v.slot_capacity, stream=sb.value)
    got = ctx.lk_windows_fetch()
    corners = ctx.good_features_fetch()[0]
    assert hip.hipStreamDestroy(sb) == 0 and hip.hipStreamDestroy(sa) == 0
    assert 100 < len(corners) <= v.slot_capacity
    ref = R.track_window(crops, corners, slots=v.slot_capacity, **R.REFERENCE)
    assert (ref[1][:len(corners)] == 2).mean() > 0.9
    same([a[0] for a in got], ref)


def test_reference_shape(ctx):
    """the two full KITTI frames as one window of two: 3000 FAST corners, 21 x 21, 3 levels, 30 iterations, 0.01"""
    a, b = O.load_kitti(0), O.load_kitti(1)
    kps = O.fast_detect(a, 20, 9, 3, 3000).astype(np.float32)
    ro, rs, re, _ = O.lk_track(a, b, kps)
    assert rs.mean() > 0.8
    ctx.lk_track_windows(np.stack([a, b]), [0], 2, kps[None])
    tracks, seen, err = ctx.lk_windows_fetch()
    assert np.array_equal(seen[0], 1 + rs.astype(np.int32))
    assert np.array_equal(bits(tracks[0, :, 0]), bits(kps))
    assert np.array_equal(bits(tracks[0, :, 1]), bits(np.where(rs[:, None] == 1, ro, 0)))
    assert np.array_equal(bits(err[0, :, 0]), bits(np.where(rs == 1, re, 0)))


def test_refusals_leave_the_previous_result(pkg, ctx, seq1, ragged_ref):
    frames, pts = seq1
    counts = np.int32(COUNTS)
    ctx.lk_track_windows(frames, FIRST, 5, pts, counts)
    bad = [
        dict(window_first=[0, 4, 2, 3]),               # 4 + 5 > 8 frames
        dict(window_first=[0, -1, 2, 3]),
        dict(window_len=1),
        dict(win=33),
        dict(max_level=8),
        dict(window_first=[], points=np.zeros((0, 301, 2), np.float32), counts=np.zeros(0, np.int32)),  # n_windows = 0
        dict(frames=np.concatenate([frames, frames[:1]])),  # 9 frames > max_batch
    ]
    for kw in bad:
        a = dict(frames=frames, window_first=FIRST, window_len=5, points=pts, counts=counts)
        a.update(kw)
        with pytest.raises(pkg.OrbxError) as e:
            ctx.lk_track_windows(a.pop("frames"), a.pop("window_first"), a.pop("window_len"), a.pop("points"),
                                 a.pop("counts"), **a)
        assert e.value.status == pkg.orbx.ERR_INVALID_ARG, kw
        same(ctx.lk_windows_fetch(), ragged_ref)
    with pytest.raises(pkg.OrbxError):
        ctx.lk_windows_fetch(3, 2)
    ctx.lk_track_windows(frames, FIRST, 5, pts, counts)
    same(ctx.lk_windows_fetch(), ragged_ref)


def test_fetch_before_any_windows_call_is_refused(pkg):
    with pkg.Context(pkg.default_params("gpu", max_width=W, max_height=H, max_batch=2)) as c:
        with pytest.raises(pkg.OrbxError):
            c.lk_windows_view()
        with pytest.raises(pkg.OrbxError):
            c.lk_windows_fetch()
