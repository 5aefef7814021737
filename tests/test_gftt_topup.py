"""Masked Shi-Tomasi detection that tops up tracked points on the GPU (orbx_good_features_topup_device and its
companions, orbx_good_features_to_track_masked) against the numpy restatement
tests/gftt_topup_ref.py.

Everything is BIT-IDENTICAL: counts, carried, the points as float bit patterns and origin, whole arrays including the
zero tail.  No tolerances."""
import ctypes as C

import numpy as np
import pytest

import gftt_ref as G
import gftt_topup_ref as T
import lk_window_ref as R

pytestmark = pytest.mark.gpu

CROPS = {"97x61": (150, 211, 400, 497), "64x48": (150, 198, 400, 464), "320x160": (100, 260, 300, 620)}
SEEDS = {"97x61": 15, "64x48": 8, "320x160": 87}
DISTANCES = [8.0, 7.5, 3.5, 1.0, 0.0]
NAN = np.float32("nan")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def kitti(pkg):
    return pkg.streams.load_kitti(0)


@pytest.fixture(scope="module")
def ctx(pkg):
    with pkg.Context(pkg.default_params("gpu", max_width=320, max_height=160, max_batch=8, nlevels=1)) as c:
        yield c


def crop_of(kitti, name):
    y0, y1, x0, x1 = CROPS[name]
    return np.ascontiguousarray(kitti[y0:y1, x0:x1])


def checkerboard(h=61, w=97):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((yy // 8) + (xx // 8)) % 2 == 0, 20, 220).astype(np.uint8)


_corner_cache = {}


def corners_of(img):
    key = (img.shape, img.tobytes())
    if key not in _corner_cache:
        _corner_cache[key] = G.good_features_to_track(img, 2000, 0.01, 8)
    return _corner_cache[key]


def fixture_seeds(img, seed=0):
    """every third corner (the strongest first) of the reference call, moved by a uniform offset within 0.49 px"""
    c = corners_of(img)[::3]
    return (c + np.random.default_rng(seed).uniform(-0.49, 0.49, c.shape)).astype(np.float32)


def pack(seed_lists, capacity=None):
    """ragged per-frame seeds as (n, capacity, 2), the unused slots NaN (dropped by rule A)"""
    capacity = capacity or max(1, max(len(s) for s in seed_lists))
    out = np.full((len(seed_lists), capacity, 2), NAN, np.float32)
    for f, s in enumerate(seed_lists):
        out[f, :len(s)] = s
    return out


def same_batch(c, frames, seed_lists, params, seen=None, seen_min=0):
    """the device entry on a batch against the restatement, whole arrays; returns the restatement's per-frame results"""
    seeds = pack(seed_lists)
    c.good_features_topup(np.stack(frames), seeds, seen, seen_min, max_corners=params[0], quality_level=params[1],
                          min_distance=params[2])
    got = c.good_features_topup_fetch()
    ref = [T.top_up(f, seeds[i], *params, seen=None if seen is None else seen[i], seen_min=seen_min, full=True)
           for i, f in enumerate(frames)]
    want = T.batch_arrays(ref, params[0])
    names = ("counts", "carried", "points", "origin")
    for g, w, name in zip(got, want, names):
        assert g.shape == w.shape, (name, g.shape, w.shape)
        assert np.array_equal(bits(g) if name == "points" else g, bits(w) if name == "points" else w), \
            (name, params, got[0], want[0], got[1], want[1])
    return ref


def same_one(c, img, seeds, params):
    pts, origin, carried = c.good_features_topup_one(img, seeds, *params)
    w_pts, w_origin, w_carried, info = T.top_up(img, seeds, *params, full=True)
    assert carried == w_carried and np.array_equal(origin, w_origin), (params, carried, w_carried, len(pts), len(w_pts))
    assert pts.shape == w_pts.shape and np.array_equal(bits(pts), bits(w_pts)), params
    return len(w_pts) - w_carried, info


# ---- parameters ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DISTANCES)
@pytest.mark.parametrize("name", list(CROPS))
def test_fixture_over_distances(ctx, kitti, name, d):
    img = crop_of(kitti, name)
    seeds = fixture_seeds(img)
    assert len(seeds) == SEEDS[name]
    new, _ = same_one(ctx, img, seeds, (2000, 0.01, d))
    print("%s d=%g: %d seeds, %d new corners" % (name, d, len(seeds), new))
    assert new > 0  # no case passes empty
    ref = same_batch(ctx, [img], [seeds], (2000, 0.01, d))
    assert len(ref[0][0]) - ref[0][2] == new


# ---- batches and slices -------------------------------------------------------------------------------------------
def batch_case(kitti):
    frames = [crop_of(kitti, "97x61"), checkerboard(), np.roll(crop_of(kitti, "97x61"), (3, 5), (0, 1))]
    seed_lists = [fixture_seeds(frames[0]), np.zeros((0, 2), np.float32), fixture_seeds(frames[2], 3)[:9]]
    return frames, seed_lists


@pytest.mark.parametrize("params", [(2000, 0.01, 8.0), (60, 0.01, 3.5), (2000, 0.02, 0.0)], ids=lambda p: "%d-%g-%g" % p)
def test_batch_of_three_frames(ctx, kitti, params):
    frames, seed_lists = batch_case(kitti)
    ref = same_batch(ctx, frames, seed_lists, params)
    assert [r[2] for r in ref] == [15, 0, 9] and all(len(r[0]) > r[2] for r in ref)
    # a frame's result does not depend on its place
    same_batch(ctx, frames[::-1], seed_lists[::-1], params)


def test_batch_in_slices_of_one_frame(pkg, kitti):
    frames, seed_lists = batch_case(kitti)
    p = pkg.default_params("gpu", max_width=97, max_height=61, max_batch=3, nlevels=1)
    with pkg.Context(p) as c:
        c.good_features_workspace_limit(1)  # one frame is always granted: three slices
        for params in ((2000, 0.01, 8.0), (60, 0.01, 3.5)):
            same_batch(c, frames, seed_lists, params)
        c.good_features_workspace_limit(0)  # the default again: the bit maps are allocated anew with the workspace
        same_batch(c, frames, seed_lists, (2000, 0.01, 8.0))


# ---- clusters -----------------------------------------------------------------------------------------------------
def test_cluster_of_seeds_in_one_cell(ctx, kitti):
    """nine usable seeds within 1.5 px of one corner -- one cell of the select grid, more than its four slots: the
    seeds never enter the grid"""
    img = crop_of(kitti, "320x160")
    c0 = corners_of(img)[0]
    c0 = np.float32([c0[0] - c0[0] % 8 + 4, c0[1] - c0[1] % 8 + 4])  # the middle of a cell of 8
    off = np.float32([[dx, dy] for dy in (-1.5, 0, 1.5) for dx in (-1.5, 0, 1.5)])
    seeds = (c0 + off).astype(np.float32)
    assert len(set(map(tuple, (seeds // 8).astype(int)))) == 1
    new, _ = same_one(ctx, img, seeds, (2000, 0.01, 8.0))
    print("cluster: %d new corners" % new)
    assert new == 277  # the restatement's count on this crop


# ---- seed positions -----------------------------------------------------------------------------------------------
def test_seed_positions_and_dropped_seeds(ctx, kitti):
    img = crop_of(kitti, "97x61")
    inf = np.float32("inf")
    seeds = np.float32([[0, 0], [96, 0], [0, 60], [96, 60],                    # the four frame corners
                        [48.5, 0], [0, 30.25], [96, 30.75], [48.25, 60],       # on the edges
                        [30.5, 30.5], [30.5, 30.5],                             # two on one pixel
                        [NAN, 5], [5, NAN], [inf, 5], [5, -inf],                # non-finite
                        [-0.001, 5], [96.001, 5], [5, -0.001], [5, 60.001],     # just outside
                        [70.75, 20.25]])
    for d in (8.0, 2.5, 0.0):
        new, _ = same_one(ctx, img, seeds, (2000, 0.01, d))
        assert new > 0
    assert list(T.usable_seeds(seeds, 97, 61)) == list(range(10)) + [18]
    # `seen` below seen_min drops a slot; origin skips it
    seen = np.full((1, len(seeds)), 5, np.int32)
    seen[0, [1, 8, 18]] = [4, 0, -3]
    ref = same_batch(ctx, [img], [seeds], (2000, 0.01, 8.0), seen, 5)
    assert list(ref[0][1][:ref[0][2]]) == [0, 2, 3, 4, 5, 6, 7, 9]


# ---- the cap ------------------------------------------------------------------------------------------------------
def test_cap(ctx, kitti):
    img = crop_of(kitti, "320x160")
    seeds = fixture_seeds(img)
    n = len(seeds)
    new, _ = same_one(ctx, img, seeds, (n, 0.01, 8.0))      # usable seeds == max_corners: no new corner
    assert new == 0
    new, _ = same_one(ctx, img, seeds, (n - 20, 0.01, 8.0))  # above: truncated in slot order
    assert new == 0
    ref = same_batch(ctx, [img, img], [seeds, seeds[:5]], (n - 20, 0.01, 8.0))
    assert list(ref[0][1]) == list(range(n - 20)) and ref[1][2] == 5 and len(ref[1][0]) == n - 20
    # the cap fills in the middle of a chunk of 64 candidates of the select walk
    new, info = same_one(ctx, img, seeds, (n + 100, 0.01, 3.5))
    assert new == 100 and len(info["indices"]) > 256 and info["kept"][99] % 64 not in (0, 63)
    new, _ = same_one(ctx, img, seeds, (n + 100, 0.01, 0.0))  # and without suppression
    assert new == 100


# ---- blocked frames and masks -------------------------------------------------------------------------------------
def test_every_pixel_blocked(ctx, kitti):
    """seeds on a lattice finer than d: the bit map is full, the masked maximum 0"""
    img = crop_of(kitti, "64x48")
    yy, xx = np.mgrid[0:48:2, 0:64:2]
    lattice = np.stack([xx.ravel(), yy.ravel()], axis=1).astype(np.float32)
    new, info = same_one(ctx, img, lattice, (2000, 0.01, 2.0))
    assert new == 0 and info["blocked"].all()
    # a flat image: no positive maximum, the seeds are carried all the same
    new, _ = same_one(ctx, np.full((48, 64), 93, np.uint8), lattice[:7], (2000, 0.01, 8.0))
    assert new == 0


def masks(img):
    h, w = img.shape
    eig = G.corner_min_eigen_val(img)
    y, x = np.unravel_index(np.argmax(eig), eig.shape)
    out = {"ones": np.full((h, w), 255, np.uint8), "zero": np.zeros((h, w), np.uint8)}
    out["half"] = out["ones"].copy()
    out["half"][:, :w // 2 + 3] = 0
    out["strongest"] = np.ones((h, w), np.uint8)  # (any non-zero byte leaves the pixel free)
    out["strongest"][y, x] = 0
    return out


@pytest.mark.parametrize("params", [(2000, 0.01, 8.0), (0, 0.001, 1.0), (5, 0.01, 0.0)], ids=lambda p: "%d-%g-%g" % p)
@pytest.mark.parametrize("name", ["97x61", "320x160", "checkerboard"])
def test_masks(ctx, kitti, name, params):
    img = checkerboard() if name == "checkerboard" else crop_of(kitti, name)
    for kind, mask in masks(img).items():
        got = ctx.good_features_to_track_masked(img, mask, *params)
        want = T.good_features_to_track_masked(img, mask, *params)
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (kind, params)
        if kind == "zero":
            assert len(want) == 0
        elif kind == "ones":
            assert np.array_equal(bits(want), bits(G.good_features_to_track(img, *params))) and len(want) > 0
        elif kind == "half":
            assert len(want) > 0 and want[:, 0].min() >= img.shape[1] // 2 + 3
        else:  # the strongest pixel is gone; on a camera frame it was the first corner
            eig = G.corner_min_eigen_val(img)
            y, x = np.unravel_index(np.argmax(eig), eig.shape)
            assert len(want) > 0 and not np.any((want[:, 0] == x) & (want[:, 1] == y))
            if name != "checkerboard":
                plain = G.good_features_to_track(img, *params)
                assert (plain[0, 0], plain[0, 1]) == (x, y) and not np.array_equal(bits(want[:1]), bits(plain[:1]))
    # a mask that is a row-strided view
    parent = np.zeros((img.shape[0], img.shape[1] + 13), np.uint8)
    parent[:, 5:5 + img.shape[1]] = masks(img)["half"]
    got = ctx.good_features_to_track_masked(img, parent[:, 5:5 + img.shape[1]], *params)
    assert np.array_equal(bits(got), bits(T.good_features_to_track_masked(img, masks(img)["half"], *params)))


# ---- seed layouts -------------------------------------------------------------------------------------------------
def test_seed_layouts(ctx, kitti):
    """the strides of an LK windows view (tracks_xy[w][slot][k], the last frame's entry) against a packed array"""
    import torch

    frames, seed_lists = batch_case(kitti)
    seeds = pack(seed_lists, 20)
    L = 4
    rng = np.random.default_rng(1)
    tracks = rng.uniform(0, 60, (3, 20, L, 2)).astype(np.float32)  # other frames' entries: never read
    tracks[:, :, L - 1] = seeds
    seen = np.full((3, 20), L, np.int32)
    seen[0, [2, 7]] = [L - 1, 1]
    params = (2000, 0.01, 8.0)
    ref = same_batch(ctx, frames, list(seeds), params, seen, L)
    packed = ctx.good_features_topup_fetch()
    t = torch.from_numpy(np.stack(frames)).cuda()
    d_tracks = torch.from_numpy(tracks).cuda()
    d_seen = torch.from_numpy(seen).cuda()
    torch.cuda.synchronize()
    ctx.good_features_topup(t, d_tracks.data_ptr() + 8 * (L - 1), d_seen, L, seed_capacity=20, seed_point_stride=2 * L,
                            seed_frame_stride=2 * L * 20, max_corners=params[0], quality_level=params[1],
                            min_distance=params[2])
    strided = ctx.good_features_topup_fetch()
    for a, b in zip(packed, strided):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert ref[0][2] == 13 and 2 not in ref[0][1] and 7 not in ref[0][1]
    # the view's pointers on the device agree with the fetch
    v = ctx.good_features_topup_view()
    assert v.n == 3 and v.slot_capacity == 2000


# ---- refusals -----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_previous_result(pkg, ctx, kitti):
    import torch

    o = pkg.orbx
    lib = o.load()
    dev = lib.orbx_good_features_topup_device
    frames, seed_lists = batch_case(kitti)
    h, w = frames[0].shape
    seeds = pack(seed_lists)
    cap = seeds.shape[1]
    t = torch.from_numpy(np.stack(frames)).cuda()
    d_seeds = torch.from_numpy(seeds).cuda()
    d_seen = torch.zeros((3, cap), dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    same_batch(ctx, frames, seed_lists, (2000, 0.01, 8.0))
    good = ctx.good_features_topup_fetch()
    v = ctx.good_features_topup_view()

    def call(ptr=t.data_ptr(), n=3, ww=w, hh=h, rs=w, fs=w * h, sxy=d_seeds.data_ptr(), ps=2, sfs=2 * cap,
             seen=d_seen.data_ptr(), seen_min=0, sc=cap, mc=2000, q=0.01, d=8.0):
        return dev(ctx._h, ptr, n, ww, hh, rs, fs, sxy, ps, sfs, seen, seen_min, sc, mc, q, d, None)

    nan, inf = float("nan"), float("inf")
    bad = [dict(ptr=None), dict(n=0), dict(n=9), dict(ww=7), dict(hh=7), dict(ww=321, rs=321), dict(hh=161),
           dict(rs=w - 1), dict(fs=w * (h - 1) + w - 1), dict(rs=1 << 26, fs=1 << 40), dict(mc=0), dict(mc=-1),
           dict(sc=0), dict(sc=-1), dict(sxy=None), dict(sxy=d_seeds.data_ptr() + 2), dict(seen=d_seen.data_ptr() + 1),
           dict(ps=1), dict(ps=0), dict(sfs=2 * cap - 1), dict(ps=4, sfs=4 * (cap - 1) + 1),
           dict(q=0.0), dict(q=1.5), dict(q=nan), dict(d=-1.0), dict(d=nan), dict(d=inf),
           dict(sxy=v.points_xy), dict(sxy=v.points_xy + 8 * 2000 * 2), dict(sxy=v.counts)]  # its own result block
    for kw in bad:
        assert call(**kw) == o.ERR_INVALID_ARG, kw
    assert call(d=64.5) == o.ERR_UNSUPPORTED and call(d=1e6) == o.ERR_UNSUPPORTED
    again = ctx.good_features_topup_fetch()
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(good, again))
    # the context stays usable; a minimum distance of 64 is accepted
    assert call(d=64.0) == o.OK
    got = ctx.good_features_topup_fetch()
    want = T.batch_arrays([T.top_up(f, seeds[i], 2000, 0.01, 64.0) for i, f in enumerate(frames)], 2000)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, want))
    # the fetch's range
    fetch = lib.orbx_good_features_topup_fetch
    three = np.full(3, -5, np.int32)
    for first, n in ((1, 3), (3, 1), (0, 4), (1, 2 ** 31 - 1), (-1, 1), (0, 0)):
        assert fetch(ctx._h, first, n, three.ctypes.data, None, None, None) == o.ERR_INVALID_ARG, (first, n)
    assert fetch(ctx._h, 0, 3, None, None, None, None) == o.ERR_INVALID_ARG and np.all(three == -5)
    assert fetch(ctx._h, 1, 2, three.ctypes.data, None, None, None) == o.OK and list(three[:2]) == list(want[0][1:])

    # the host entries
    img = frames[0]
    one = lib.orbx_good_features_topup
    SENT = np.float32(-7.5)
    pts = np.full((64, 2), SENT, np.float32)
    org = np.full(64, -9, np.int32)
    cnt, car = C.c_int(-123), C.c_int(-321)
    s0 = np.ascontiguousarray(seed_lists[0])

    def call_one(image=img.ctypes.data, ww=w, hh=h, stride=w, sxy=s0.ctypes.data, ns=len(s0), mc=64, q=0.01, d=8.0,
                 p=pts.ctypes.data, og=org.ctypes.data, capacity=64, count=C.byref(cnt), carried=C.byref(car)):
        return one(ctx._h, image, ww, hh, stride, sxy, ns, mc, q, d, p, og, capacity, count, carried)

    for kw in (dict(image=None), dict(ww=7), dict(stride=w - 1), dict(sxy=None), dict(ns=-1), dict(mc=0), dict(q=0.0),
               dict(d=-0.5), dict(p=None), dict(og=None), dict(capacity=-1), dict(count=None), dict(carried=None)):
        assert call_one(**kw) == o.ERR_INVALID_ARG, kw
    assert call_one(d=64.5) == o.ERR_UNSUPPORTED
    assert cnt.value == -123 and car.value == -321 and np.all(pts == SENT) and np.all(org == -9)
    need = len(T.top_up(img, s0, 64, 0.01, 8.0)[0])
    assert 15 < need <= 64
    assert call_one(capacity=need - 1) == o.ERR_CAPACITY and cnt.value == need and np.all(pts == SENT)
    assert call_one(capacity=need) == o.OK and cnt.value == need and car.value == 15 and np.all(pts[need:] == SENT)
    assert call_one(sxy=None, ns=0) == o.OK and car.value == 0  # no seeds at all
    masked = lib.orbx_good_features_to_track_masked
    mask = np.full((h, w), 255, np.uint8)
    pts[...] = SENT
    cnt.value = -123
    for m, ms, d in ((None, w, 8.0), (mask.ctypes.data, w - 1, 8.0), (mask.ctypes.data, w, -1.0)):
        assert masked(ctx._h, img.ctypes.data, w, h, w, m, ms, 0, 0.01, d, pts.ctypes.data, 64, C.byref(cnt)) == \
            o.ERR_INVALID_ARG
    assert masked(ctx._h, img.ctypes.data, w, h, w, mask.ctypes.data, w, 0, 0.01, 64.5, pts.ctypes.data, 64,
                  C.byref(cnt)) == o.ERR_UNSUPPORTED
    assert cnt.value == -123 and np.all(pts == SENT)
    need = len(G.good_features_to_track(img, 0, 0.01, 3.0))
    assert need > 64
    assert masked(ctx._h, img.ctypes.data, w, h, w, mask.ctypes.data, w, 0, 0.01, 3.0, pts.ctypes.data, 64,
                  C.byref(cnt)) == o.ERR_CAPACITY and cnt.value == need and np.all(pts == SENT)


def test_fetch_before_any_topup_is_refused(pkg):
    p = pkg.default_params("gpu", max_width=64, max_height=48, nlevels=1)
    with pkg.Context(p) as c:
        with pytest.raises(pkg.OrbxError) as e:
            c.good_features_topup_fetch()
        assert e.value.status == pkg.orbx.ERR_INVALID_ARG


# ---- other blocks -------------------------------------------------------------------------------------------------
def test_the_plain_block_and_the_lk_block_are_untouched(ctx, kitti):
    frames = R.shifted_frames(1, 96, 128, 3, (-2.4, 1.7))
    pts = R.box_points(1, 100, 96, 128)[None]
    ctx.good_features_batch(np.stack(batch_case(kitti)[0]), 500, 0.01, 8.0)
    ctx.lk_track_windows(frames, [0], 3, pts)
    gf_before, lk_before = ctx.good_features_fetch(), ctx.lk_windows_fetch()
    assert len(gf_before[0]) > 20 and (lk_before[1] == 3).sum() > 20
    same_batch(ctx, *batch_case(kitti), (2000, 0.01, 8.0))
    img = crop_of(kitti, "64x48")
    ctx.good_features_to_track_masked(img, masks(img)["half"], 0, 0.01, 2.0)
    gf_after, lk_after = ctx.good_features_fetch(), ctx.lk_windows_fetch()
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(gf_before, gf_after))
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(lk_before, lk_after))


# ---- one chain on the device --------------------------------------------------------------------------------------
def test_chain_detect_track_topup_track(ctx):
    """corners of frame 0 -> LK window over frames 0..2 -> top-up on frame 2 straight from the LK view -> LK window
    over frames 2..4 straight from the top-up view: nothing visits the host.  Against the same chain through the numpy
    restatements; origin maps the second window's slots back to the first's."""
    import torch

    Lw, cap, params = 3, 300, (300, 0.01, 6.0)
    frames = R.shifted_frames(1, 96, 128, 5, (-2.4, 1.7))
    t = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    ctx.good_features_batch(t[:1], *params)
    g = ctx.good_features_view()
    assert g.slot_capacity == cap
    ctx.lk_track_windows(t, [0], Lw, g.corners_xy, g.counts, slot_capacity=cap)
    lk = ctx.lk_windows_view()
    ctx.good_features_topup(t[Lw - 1:Lw], lk.tracks_xy + 8 * (Lw - 1), lk.seen, Lw, seed_capacity=cap,
                            seed_point_stride=2 * Lw, seed_frame_stride=2 * Lw * cap, max_corners=params[0],
                            quality_level=params[1], min_distance=params[2])
    tv = ctx.good_features_topup_view()
    assert tv.slot_capacity == cap
    first = ctx.lk_windows_fetch()
    ctx.lk_track_windows(t, [Lw - 1], Lw, tv.points_xy, tv.counts, slot_capacity=cap)
    second = ctx.lk_windows_fetch()
    counts, carried, points, origin = ctx.good_features_topup_fetch()

    # the same chain on the host
    corners = G.good_features_to_track(frames[0], *params)
    assert 40 < len(corners) < cap
    r1 = R.track_window(frames[:Lw], corners, slots=cap, **R.REFERENCE)
    for a, b in zip((x[0] for x in first), r1):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    w_pts, w_origin, w_carried = T.top_up(frames[Lw - 1], r1[0][:, Lw - 1], *params, seen=r1[1], seen_min=Lw)
    want = T.batch_arrays([(w_pts, w_origin, w_carried)], cap)
    for a, b in zip((counts, carried, points, origin), want):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    alive = int((r1[1][:len(corners)] == Lw).sum())
    print("chain: %d corners, %d tracked through the window, %d carried, %d new" % (len(corners), alive, w_carried,
                                                                                    len(w_pts) - w_carried))
    # some tracks ended or left the frame (rule A drops those), and their places are filled
    assert 0 < w_carried < len(corners) and w_carried <= alive and len(w_pts) > w_carried
    r2 = R.track_window(frames[Lw - 1:], w_pts, slots=cap, **R.REFERENCE)
    for a, b in zip((x[0] for x in second), r2):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # origin joins the windows: a carried slot of the second window starts where its first-window slot ended
    for i in range(w_carried):
        assert np.array_equal(bits(second[0][0, i, 0]), bits(first[0][0, origin[0, i], Lw - 1]))
        assert first[1][0, origin[0, i]] == Lw
    assert np.all(origin[0, w_carried:] == -1)
