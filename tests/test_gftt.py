"""Batched Shi-Tomasi corner detection on the GPU (orbx_corner_min_eigen_val, orbx_good_features_to_track,
orbx_good_features_batch_device) against the numpy restatement tests/gftt_ref.py.

Everything is BIT-IDENTICAL: the response map as float bit patterns, and the count, order and coordinates of the
corners.  No tolerances."""
import ctypes as C

import numpy as np
import pytest

import gftt_ref as G

pytestmark = pytest.mark.gpu

W, H = 1241, 376
# maxCorners, qualityLevel, minDistance
PARAMS = [
    (2000, 0.01, 8.0),   # the reference's values
    (200, 0.01, 3.5),    # the cap is reached on the 320 x 160 crop
    (0, 0.001, 1.0),     # no limit, cell = 1
    (5, 0.01, 0.0),      # no suppression
    (0, 0.01, 8.5),      # cvRound half-even: cell 8
    (0, 0.3, 2.0),
    (0, 0.01, 12.5),
]
CROPS = {"97x61": (150, 211, 400, 497), "64x48": (150, 198, 400, 464), "320x160": (100, 260, 300, 620)}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def kitti(pkg):
    return pkg.streams.load_kitti(0)


@pytest.fixture(scope="module")
def ctx(pkg):
    with pkg.Context(pkg.default_params("gpu", max_width=W, max_height=H, max_batch=8)) as c:
        yield c


def crop_of(kitti, name):
    y0, y1, x0, x1 = CROPS[name]
    return np.ascontiguousarray(kitti[y0:y1, x0:x1])


def checkerboard(h=61, w=97):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((yy // 8) + (xx // 8)) % 2 == 0, 20, 220).astype(np.uint8)


def rectangle(h=48, w=64):
    img = np.zeros((h, w), np.uint8)
    img[16:32, 20:44] = 255
    return img


def noise(h=61, w=97, seed=7):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


_ref_cache = {}


def ref(img, params):
    """the restatement's corners, computed once per (image, parameters)"""
    key = (img.shape, img.tobytes(), params)
    if key not in _ref_cache:
        _ref_cache[key] = G.good_features_to_track(np.ascontiguousarray(img), *params, full=True)
    return _ref_cache[key]


def same_corners(got, img, params, min_candidates=None):
    want, full = ref(img, params)
    assert got.dtype == np.float32 and got.shape == want.shape, (got.shape, want.shape, params)
    assert np.array_equal(bits(got), bits(want)), params
    if min_candidates is not None:  # the case must not pass empty
        assert len(full["indices"]) >= min_candidates, len(full["indices"])


# ---- response map -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["97x61", "64x48", "full"])
def test_response_map(ctx, kitti, name):
    img = kitti if name == "full" else crop_of(kitti, name)
    got = ctx.corner_min_eigen_val(img)
    want = G.corner_min_eigen_val(img)
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
    assert want.max() > 0.01


def test_response_map_strided_unaligned_view(ctx, kitti):
    """a region of a larger image at an odd byte offset with an odd row stride, garbage all around"""
    parent = np.random.default_rng(3).integers(0, 256, (70, 131), dtype=np.uint8)
    view = parent[5:5 + 61, 3:3 + 97]
    view[...] = crop_of(kitti, "97x61")
    assert view.strides == (131, 1) and not view.flags["C_CONTIGUOUS"]
    got = ctx.corner_min_eigen_val(view)
    assert np.array_equal(bits(got), bits(G.corner_min_eigen_val(crop_of(kitti, "97x61"))))
    same_corners(ctx.good_features_to_track(view, 2000, 0.01, 8.0), crop_of(kitti, "97x61"), (2000, 0.01, 8.0), 100)


# ---- corners ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", PARAMS, ids=lambda p: "%d-%g-%g" % p)
@pytest.mark.parametrize("name", list(CROPS))
def test_corners_on_crops(ctx, kitti, name, params):
    img = crop_of(kitti, name)
    same_corners(ctx.good_features_to_track(img, *params), img, params, 20)
    if name == "320x160" and params[0] == 200:
        assert len(ref(img, params)[0]) == 200  # the cap is reached


def test_corners_on_the_full_frame(ctx, kitti):
    """more than 64 chunks of candidates, fewer corners than the cap: the whole sorted list is consumed"""
    params = (2000, 0.01, 8.0)
    same_corners(ctx.good_features_to_track(kitti, *params), kitti, params, 2000)
    assert len(ref(kitti, params)[0]) < 2000


LDS_KEYS = 8192  # k_gftt_select sorts lists up to this length in LDS, longer ones in place in the key pool


@pytest.mark.parametrize("params", [(0, 0.001, 1.0), (2000, 0.001, 8.0)], ids=lambda p: "%d-%g-%g" % p)
def test_candidate_lists_beyond_the_lds_sort(ctx, kitti, params):
    """the full frame at quality 0.001: more than 8192 candidates, so the sort runs in the global key pool and the
    walk reads the keys from there; every candidate accepted (distance 1), and the cap reached (distance 8)"""
    same_corners(ctx.good_features_to_track(kitti, *params), kitti, params, LDS_KEYS + 1)
    assert len(ref(kitti, params)[0]) >= 2000


def test_batch_mixes_long_and_short_candidate_lists(ctx, kitti):
    """one launch whose frames sort in the key pool (> 8192 candidates), in LDS, and not at all (a flat frame)"""
    half = kitti.copy()
    half[150:] = 128
    frames = [kitti, half, np.full_like(kitti, 77), np.roll(kitti, (5, 9), (0, 1))]
    for params in ((2000, 0.001, 8.0), (20000, 0.001, 1.0)):
        n = [len(ref(f, params)[1]["indices"]) for f in frames]
        assert n[0] > LDS_KEYS and 64 < n[1] <= LDS_KEYS and n[2] == 0 and n[3] > LDS_KEYS, n
        check_batch(ctx, frames, params)
        check_batch(ctx, frames[::-1], params)


@pytest.mark.parametrize("params", [(2000, 0.01, 8.0), (0, 0.01, 2.0), (0, 0.05, 1.5)], ids=lambda p: "%d-%g-%g" % p)
@pytest.mark.parametrize("name", ["checkerboard", "rectangle", "flat", "noise"])
def test_synthetic_images(ctx, name, params):
    """checkerboard: hundreds of candidates tied in value (the order is the index's); noise: many weak maxima, lists
    that cross several 64-candidate chunks; flat: no corner at all"""
    img = {"checkerboard": checkerboard(), "rectangle": rectangle(), "flat": np.full((48, 64), 93, np.uint8),
           "noise": noise()}[name]
    got = ctx.good_features_to_track(img, *params)
    same_corners(got, img, params)
    n = len(ref(img, params)[1]["indices"])
    assert n == 0 if name == "flat" else n >= 4
    if name == "noise":
        assert n > 3 * 64
    assert np.array_equal(bits(ctx.corner_min_eigen_val(img)), bits(G.corner_min_eigen_val(img)))


@pytest.mark.parametrize("h,w", [(8, 8), (64, 9), (9, 64), (20, 65), (33, 121)])
def test_geometry_edges(ctx, h, w):
    """the smallest frame, one-strip frames in either direction, a width of 65 (one lane into the second wave of the
    candidate pass), a width of 121 (one column into the third 60-column strip of the response pass)"""
    img = noise(h, w, seed=h * 131 + w)
    assert np.array_equal(bits(ctx.corner_min_eigen_val(img)), bits(G.corner_min_eigen_val(img)))
    for params in ((0, 0.01, 1.5), (0, 0.01, 0.0), (3, 0.2, 3.0)):
        same_corners(ctx.good_features_to_track(img, *params), img, params)


# ---- batches ------------------------------------------------------------------------------------------------------
def batch_frames(kitti):
    return [crop_of(kitti, "97x61"), np.full((61, 97), 200, np.uint8), checkerboard(), noise(),
            rectangle(61, 97)]


def check_batch(c, frames, params, device_frames=None):
    import torch

    t = torch.from_numpy(np.stack(frames)).cuda() if device_frames is None else device_frames
    torch.cuda.synchronize()
    c.good_features_batch(t, *params)
    got = c.good_features_fetch()
    assert len(got) == len(frames)
    for g, f in zip(got, frames):
        same_corners(g, f, params)


BATCH_PARAMS = [(2000, 0.01, 8.0), (40, 0.01, 2.0), (2000, 0.02, 0.0)]


@pytest.mark.parametrize("params", BATCH_PARAMS, ids=lambda p: "%d-%g-%g" % p)
def test_batch_equals_single_frames(ctx, kitti, params):
    frames = batch_frames(kitti)
    for f in frames:  # the single-frame entry on each of them
        same_corners(ctx.good_features_to_track(f, *params), f, params)
    check_batch(ctx, frames, params)
    check_batch(ctx, frames[::-1], params)  # a frame's result does not depend on its place
    check_batch(ctx, frames[3:4], params)   # n = 1
    assert sum(len(ref(f, params)[0]) for f in frames) > 50


class _DeviceArray:
    """a device address as something torch.as_tensor reads"""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 2}


def test_device_view_and_callers_streams(ctx, kitti):
    """orbx_good_features_results_device: counts at `counts`, frame f's corners at corners_xy + f * slot_capacity * 2,
    read on the GPU through the view's pointers and compared with the fetch.  The batches run on two streams of the
    caller in turn: the second call, the view's reader and the fetch follow the event behind the batch."""
    import torch

    frames = batch_frames(kitti)
    t = torch.from_numpy(np.stack(frames)).cuda()
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for k, params in enumerate(((2000, 0.01, 8.0), (30, 0.01, 2.0), (2000, 0.01, 3.0))):
        s = streams[k % 2]
        ctx.good_features_batch(t, *params, stream=s.cuda_stream)
        v = ctx.good_features_view()
        assert v.n == len(frames) and v.slot_capacity == min(params[0], 95 * 59)
        with torch.cuda.stream(s):  # in order behind the batch
            counts = torch.as_tensor(_DeviceArray(v.counts, (v.n,), "<i4"), device="cuda").cpu().numpy()
            xy = torch.as_tensor(_DeviceArray(v.corners_xy, (v.n, v.slot_capacity, 2), "<f4"), device="cuda")
            xy = xy.cpu().numpy()
        got = ctx.good_features_fetch()
        for f, frame in enumerate(frames):
            same_corners(got[f], frame, params)
            assert counts[f] == len(got[f]) and np.array_equal(bits(xy[f, :counts[f]]), bits(got[f]))


def test_batch_strided_frames_with_garbage_gaps(ctx, kitti):
    """regions of a parent buffer, as in test_batch_inputs.py: odd base, odd row stride, gaps between the frames;
    the bytes around the regions are 0x00, then 0xff, and never matter"""
    import torch

    frames = np.stack(batch_frames(kitti))
    n, h, w = frames.shape
    base, rs, fs = 3, 131, 131 * 63 + 5
    for fill in (0x00, 0xFF):
        buf = np.full(base + (n - 1) * fs + (h - 1) * rs + w + 3, fill, np.uint8)
        np.lib.stride_tricks.as_strided(buf[base:], shape=(n, h, w), strides=(fs, rs, 1))[...] = frames
        t = torch.from_numpy(buf).cuda()
        view = torch.as_strided(t, (n, h, w), (fs, rs, 1), base)
        check_batch(ctx, list(frames), (2000, 0.01, 8.0), device_frames=view)


def test_batch_on_a_pipelined_context(pkg, kitti):
    """pipelined ORB batches before and after: the good-features batch has its own workspace and result block"""
    import torch

    frames = batch_frames(kitti)
    p = pkg.default_params("gpu", max_width=97, max_height=61, max_batch=5, nlevels=2, nfeatures=200)
    with pkg.Context(p) as c:
        c.set_pipelined_batches(True)
        t = torch.from_numpy(np.stack(frames)).cuda()
        torch.cuda.synchronize()
        for _ in range(3):
            c.batch_device(t.data_ptr(), 5, 97, 61)
            check_batch(c, frames, (2000, 0.01, 8.0), device_frames=t)
        c.wait()


def test_batch_larger_than_one_workspace_slice(pkg, kitti):
    """a workspace bound of two frames: five frames run as slices of 2, 2 and 1 with identical results"""
    frames = batch_frames(kitti)
    p = pkg.default_params("gpu", max_width=97, max_height=61, max_batch=5, nlevels=1)
    with pkg.Context(p) as c:
        c.good_features_workspace_limit(int(2.5 * 16 * 97 * 61))
        for params in BATCH_PARAMS:
            check_batch(c, frames, params)
        c.good_features_workspace_limit(1)  # one frame is always granted: five slices
        check_batch(c, frames, (2000, 0.01, 8.0))
        c.good_features_workspace_limit(0)  # the default again
        check_batch(c, frames, (2000, 0.01, 8.0))


def test_orb_state_is_untouched(ctx, kitti):
    """results, matches and poses of an ORB batch fetched before and after a good-features batch are identical"""
    import torch

    frames = np.stack([np.ascontiguousarray(kitti[100 + 2 * i:260 + 2 * i, 300 + 3 * i:620 + 3 * i]) for i in range(3)])
    K = np.array([[718.856, 0, 160.0], [0, 718.856, 80.0], [0, 0, 1]])
    t = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    cap = ctx.plan(320, 160)["out_capacity"]

    def snapshot():
        out = [ctx.batch_fetch(0, 3, cap)]
        out += [ctx.batch_match_fetch(pair, cap) for pair in (0, 1)]
        out.append(ctx.batch_pose_fetch())
        return out

    ctx.batch_device(t.data_ptr(), 3, 320, 160)
    ctx.batch_match_consecutive(0.8)
    ctx.batch_pose_consecutive(K)
    before = snapshot()
    assert before[0]["counts"].min() > 50 and len(before[1][0]) > 10
    check_batch(ctx, list(frames), (2000, 0.01, 8.0))
    same_corners(ctx.good_features_to_track(frames[0], 0, 0.01, 3.0), frames[0], (0, 0.01, 3.0))
    after = snapshot()
    for k in before[0]:
        assert np.array_equal(before[0][k], after[0][k]), k
    for pair in (1, 2):
        assert all(np.array_equal(a, b) for a, b in zip(before[pair], after[pair]))
    for k in before[3]:
        assert np.array_equal(before[3][k], after[3][k]), k


# ---- refusals -----------------------------------------------------------------------------------------------------
def _entries(pkg):
    lib = pkg.orbx.load()
    return lib.orbx_good_features_to_track, lib.orbx_good_features_batch_device, lib.orbx_corner_min_eigen_val


def test_refusals(pkg, ctx, kitti):
    import torch

    o = pkg.orbx
    one, batch, eig = _entries(pkg)
    img = crop_of(kitti, "97x61")
    h, w = img.shape
    ip = img.ctypes.data
    SENT = np.float32(-7.5)
    out = np.full((64, 2), SENT, np.float32)
    cnt = C.c_int(-123)

    def call_one(image=ip, ww=w, hh=h, stride=w, mc=10, q=0.01, d=8.0, corners=out.ctypes.data, capacity=64,
                 count=C.byref(cnt)):
        return one(ctx._h, image, ww, hh, stride, mc, q, d, corners, capacity, count)

    nan, inf = float("nan"), float("inf")
    bad = [dict(image=None), dict(ww=7), dict(hh=7), dict(ww=W + 1, stride=W + 1), dict(hh=H + 1), dict(stride=w - 1),
           dict(q=0.0), dict(q=-0.1), dict(q=1.0000001), dict(q=nan), dict(q=inf), dict(d=-0.5), dict(d=nan),
           dict(d=inf), dict(capacity=-1), dict(corners=None), dict(count=None)]
    for kw in bad:
        assert call_one(**kw) == o.ERR_INVALID_ARG, kw
    # the one limit: a minimum distance beyond ORBX_GFTT_MAX_MIN_DISTANCE
    assert call_one(d=65536.5) == o.ERR_UNSUPPORTED
    assert cnt.value == -123 and np.all(out == SENT)  # nothing is written on error
    assert call_one(d=65536.0, mc=0) == o.OK and cnt.value == 1  # at the limit: the strongest corner alone
    want = ref(img, (0, 0.01, 65536.0))[0]
    assert len(want) == 1 and np.array_equal(bits(out[:1]), bits(want)) and np.all(out[1:] == SENT)
    # capacity: the required count comes back, the buffer stays as it was
    out[...] = SENT
    need = len(ref(img, (0, 0.01, 8.0))[0])
    assert need > 3
    assert call_one(mc=0, capacity=3) == o.ERR_CAPACITY and cnt.value == need and np.all(out == SENT)
    assert call_one(mc=0, capacity=0, corners=None) == o.ERR_CAPACITY and cnt.value == need
    assert call_one(mc=0, capacity=need) == o.OK and cnt.value == need
    assert np.array_equal(bits(out[:need]), bits(ref(img, (0, 0.01, 8.0))[0])) and np.all(out[need:] == SENT)
    assert call_one(mc=3, capacity=3) == o.OK and cnt.value == 3  # max_corners within the capacity

    # the stage entry
    m = np.full((h, w), SENT, np.float32)
    for args in ((None, w, h, w, m.ctypes.data), (ip, 7, h, w, m.ctypes.data), (ip, w, h, w - 1, m.ctypes.data),
                 (ip, w, h, w, None), (ip, W + 1, h, W + 1, m.ctypes.data)):
        assert eig(ctx._h, *args) == o.ERR_INVALID_ARG, args
    assert np.all(m == SENT)

    # the batch entry
    frames = np.stack([img, img])
    t = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    ctx.good_features_batch(t, 2000, 0.01, 8.0)
    good = ctx.good_features_fetch()

    def call_batch(ptr=t.data_ptr(), n=2, ww=w, hh=h, rs=w, fs=w * h, mc=2000, q=0.01, d=8.0):
        return batch(ctx._h, ptr, n, ww, hh, rs, fs, mc, q, d, None)

    bad = [dict(ptr=None), dict(n=0), dict(n=9), dict(ww=7), dict(hh=7), dict(ww=W + 1, rs=W + 1), dict(hh=H + 1),
           dict(rs=w - 1), dict(fs=w * (h - 1) + w - 1), dict(rs=1 << 26, fs=1 << 40), dict(mc=0), dict(mc=-1),
           dict(q=0.0), dict(q=1.5), dict(q=nan), dict(d=-1.0), dict(d=nan), dict(d=inf)]
    for kw in bad:
        assert call_batch(**kw) == o.ERR_INVALID_ARG, kw
    assert call_batch(d=1e6) == o.ERR_UNSUPPORTED
    # a refused call leaves the last batch's results where they were, and the context usable
    again = ctx.good_features_fetch()
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(good, again))
    assert call_batch() == o.OK
    for g in ctx.good_features_fetch():
        same_corners(g, img, (2000, 0.01, 8.0))
    fetch = pkg.orbx.load().orbx_good_features_fetch
    two = np.full(2, -5, np.int32)
    for first, n in ((1, 2), (2, 1), (0, 3), (1, 2 ** 31 - 1), (-1, 1), (0, 0)):  # beyond the batch
        assert fetch(ctx._h, first, n, two.ctypes.data, None) == o.ERR_INVALID_ARG, (first, n)
    assert fetch(ctx._h, 0, 2, None, None) == o.ERR_INVALID_ARG and np.all(two == -5)


def test_fetch_before_any_batch_is_refused(pkg):
    p = pkg.default_params("gpu", max_width=64, max_height=48, nlevels=1)
    with pkg.Context(p) as c:
        with pytest.raises(pkg.OrbxError) as e:
            c.good_features_fetch()
        assert e.value.status == pkg.orbx.ERR_INVALID_ARG


# ---- the two stages compose ---------------------------------------------------------------------------------------
def test_chain_with_lk(ctx, kitti):
    """corners of the 320 x 160 crop fed to the LK tracker between the crop and its np.roll by (3, 1): every corner
    farther than the LK window from the border is tracked to within the tracker's own epsilon"""
    img = crop_of(kitti, "320x160")
    nxt = np.roll(img, (3, 1), axis=(0, 1))
    pts = ctx.good_features_to_track(img, 500, 0.01, 8.0)
    same_corners(pts, img, (500, 0.01, 8.0), 200)
    win, eps = 21, 0.01
    out, status, _ = ctx.lk_track(img, nxt, pts, win=win, max_level=3, max_iters=30, epsilon=eps)
    inner = (pts[:, 0] > win) & (pts[:, 0] < 320 - 1 - win) & (pts[:, 1] > win) & (pts[:, 1] < 160 - 1 - win)
    assert inner.sum() > 50
    err = np.hypot(out[:, 0] - (pts[:, 0] + 1), out[:, 1] - (pts[:, 1] + 3))
    print("LK chain: %d inner corners, tracked %d, worst error %.5f" % (inner.sum(), status[inner].sum(),
                                                                       err[inner].max()))
    assert np.all(status[inner] == 1)
    assert err[inner].max() <= eps
