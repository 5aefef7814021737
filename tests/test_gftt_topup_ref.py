"""Pins tests/gftt_topup_ref.py, the numpy restatement of the masked detection that tops up tracked points (DESIGN.md
§9 rank 12, rules A-F): against the plain restatement where nothing is blocked, and by brute force over all pixels on
the properties the rules promise.  No GPU."""
import numpy as np
import pytest

import gftt_ref as G
import gftt_topup_ref as T

CROPS = {"97x61": (150, 211, 400, 497), "64x48": (150, 198, 400, 464), "320x160": (100, 260, 300, 620)}
SEEDS = {"97x61": 15, "64x48": 8, "320x160": 87}
DISTANCES = [8.0, 7.5, 3.5, 1.0, 0.0]


@pytest.fixture(scope="module")
def kitti(pkg):
    return pkg.streams.load_kitti(0)


def crop_of(kitti, name):
    y0, y1, x0, x1 = CROPS[name]
    return np.ascontiguousarray(kitti[y0:y1, x0:x1])


def fixture_seeds(img, seed=0):
    """every third corner (the strongest first) of the reference call, moved by a uniform offset within 0.49 px"""
    c = G.good_features_to_track(img, 2000, 0.01, 8)[::3]
    return (c + np.random.default_rng(seed).uniform(-0.49, 0.49, c.shape)).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("params", [(2000, 0.01, 8.0), (0, 0.001, 1.0), (5, 0.01, 0.0), (0, 0.01, 3.5)])
@pytest.mark.parametrize("name", list(CROPS))
def test_nothing_blocked_is_the_plain_detector(kitti, name, params):
    img = crop_of(kitti, name)
    want = G.good_features_to_track(img, *params)
    got = T.good_features_to_track_masked(img, np.full(img.shape, 255, np.uint8), *params)
    assert len(want) > 0 and got.shape == want.shape and np.array_equal(bits(got), bits(want))
    if params[0] > 0:
        pts, origin, carried = T.top_up(img, np.zeros((0, 2), np.float32), *params)
        assert carried == 0 and np.all(origin == -1) and np.array_equal(bits(pts), bits(want))


@pytest.mark.parametrize("d", DISTANCES)
@pytest.mark.parametrize("name", list(CROPS))
def test_brute_force_properties(kitti, name, d):
    img = crop_of(kitti, name)
    h, w = img.shape
    seeds = fixture_seeds(img)
    assert len(seeds) == SEEDS[name]
    for cap in (2000, len(seeds) + 7):
        pts, origin, carried, info = T.top_up(img, seeds, cap, 0.01, d, full=True)
        new = pts[carried:]
        print("%s d=%g cap=%d: %d seeds, %d new corners of %d candidates" % (name, d, cap, carried, len(new),
                                                                            len(info["indices"])))
        assert carried == len(seeds) and len(new) > 0  # no case passes empty
        assert np.array_equal(origin[:carried], np.arange(carried)) and np.all(origin[carried:] == -1)
        assert np.array_equal(bits(pts[:carried]), bits(seeds))
        assert len(pts) <= cap
        # brute force over all pixels, in float64 on the float32 values (exact: squares of 24-bit numbers, one sum)
        nx, ny = new[:, 0].astype(np.int64), new[:, 1].astype(np.int64)
        d2 = np.float32(np.float64(d) * np.float64(d))
        X, Y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
        blocked = np.zeros((h, w), bool)
        if d >= 1:
            for sx, sy in seeds:
                dx, dy = X - sx, Y - sy
                blocked |= (dx * dx + dy * dy) < d2
        assert np.array_equal(blocked, info["blocked"])
        assert not blocked[ny, nx].any()  # no new corner is blocked
        if d >= 1:
            # (pixel centres closer than d to a seed are blocked: a looser, float64 statement of the same)
            far = np.hypot(new[:, None, 0].astype(np.float64) - seeds[None, :, 0],
                           new[:, None, 1].astype(np.float64) - seeds[None, :, 1])
            assert far.min() >= d * (1 - 1e-6)
            dist2 = (nx[:, None] - nx[None, :]) ** 2 + (ny[:, None] - ny[None, :]) ** 2
            np.fill_diagonal(dist2, 1 << 40)
            assert dist2.min() >= np.float64(d2)  # new corners are mutually not closer than d
        # every candidate that was not accepted has its reason
        idx, kept = info["indices"], info["kept"]
        assert not blocked.reshape(-1)[idx].any()
        cx, cy = idx % w, idx // w
        is_kept = np.zeros(len(idx), bool)
        is_kept[kept] = True
        full = len(new) == cap - carried
        for i in np.flatnonzero(~is_kept):
            if full and i > kept[-1]:
                continue  # came after the cap filled
            assert d >= 1
            earlier = kept[kept < i]
            assert np.any((cx[i] - cx[earlier]) ** 2 + (cy[i] - cy[earlier]) ** 2 < np.float64(d2)), (d, i)
        if cap == 2000:
            assert not full
        else:
            assert full and len(pts) == cap


def test_the_masked_maximum_differs_when_the_strongest_corner_is_seeded(kitti):
    img = crop_of(kitti, "320x160")
    seeds = fixture_seeds(img)
    eig = G.corner_min_eigen_val(img)
    y, x = np.unravel_index(np.argmax(eig), eig.shape)
    assert abs(seeds[0, 0] - x) < 0.5 and abs(seeds[0, 1] - y) < 0.5  # the strongest corner is the first seed
    blocked = T.blocked_by_seeds(seeds, 320, 160, 1.0)
    assert blocked[y, x] and 0 < T.masked_max(eig, blocked) < eig.max()
    # a lower threshold: more candidates than the plain detector has, though some pixels are blocked (rule D)
    n_plain = len(G.candidates(eig, 0.01)[1])
    n_masked = len(T.candidates(eig, 0.01, blocked)[1])
    assert n_masked > n_plain, (n_masked, n_plain)
    # min_distance < 1: nothing is blocked, the frame maximum holds
    assert not T.blocked_by_seeds(seeds, 320, 160, 0.99).any()
    assert len(T.top_up(img, seeds, 2000, 0.01, 0.0)[0]) - len(seeds) == n_plain


def test_all_blocked_or_no_positive_maximum_gives_no_new_corner(kitti):
    img = crop_of(kitti, "64x48")
    assert len(T.good_features_to_track_masked(img, np.zeros(img.shape, np.uint8), 0, 0.01, 8.0)) == 0
    yy, xx = np.mgrid[0:48:2, 0:64:2]
    lattice = np.stack([xx.ravel(), yy.ravel()], axis=1).astype(np.float32)
    pts, origin, carried, info = T.top_up(img, lattice, 5000, 0.01, 2.0, full=True)
    assert info["blocked"].all() and carried == len(lattice) == len(pts)
    flat = np.full((48, 64), 93, np.uint8)
    assert len(T.top_up(flat, lattice[:3], 100, 0.01, 8.0)[0]) == 3


def test_seed_rules(kitti):
    """rule A: live and usable; rule B: slot order, truncation at max_corners"""
    img = crop_of(kitti, "97x61")
    nan, inf = np.float32("nan"), np.float32("inf")
    seeds = np.array([[5.5, 5.5], [nan, 3], [96.0, 60.0], [96.00001, 10], [3, inf], [0, 0], [-1e-6, 4], [3, -inf],
                      [40.25, 60.0], [40, 60.5], [20, 20], [20, 20]], np.float32)
    assert list(T.usable_seeds(seeds, 97, 61)) == [0, 2, 5, 8, 10, 11]
    seen = np.array([5, 5, 4, 5, 5, 5, 5, 5, 6, 5, 0, 5], np.int32)
    assert list(T.usable_seeds(seeds, 97, 61, seen, 5)) == [0, 5, 8, 11]
    pts, origin, carried = T.top_up(img, seeds, 2000, 0.01, 8.0, seen, 5)
    assert carried == 4 and list(origin[:4]) == [0, 5, 8, 11] and np.array_equal(bits(pts[:4]), bits(seeds[[0, 5, 8, 11]]))
    pts, origin, carried = T.top_up(img, seeds, 3, 0.01, 8.0)
    assert carried == 3 and len(pts) == 3 and list(origin) == [0, 2, 5]
    counts, car, P, O = T.batch_arrays([T.top_up(img, seeds, 6, 0.01, 8.0), T.top_up(img, seeds[:1], 6, 0.01, 64.0)], 6)
    assert list(car) == [6, 1] and counts[0] == 6 and 1 <= counts[1] < 6
    assert np.all(P[1, counts[1]:] == 0) and np.all(O[1, counts[1]:] == -1) and np.all(O[1, 1:] == -1)
