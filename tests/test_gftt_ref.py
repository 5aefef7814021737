"""Pins tests/gftt_ref.py, the numpy restatement of the library's Shi-Tomasi corner detection (DESIGN.md §9 rank 8,
rules 1-6), on inputs whose answers are known, on the properties greedy selection must have, and against a float64
evaluation of rule 1.  No GPU."""
import numpy as np
import pytest

import gftt_ref as G


def checkerboard(h=61, w=97):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((yy // 8) + (xx // 8)) % 2 == 0, 20, 220).astype(np.uint8)


def rectangle():
    img = np.zeros((48, 64), np.uint8)
    img[16:32, 20:44] = 255
    return img


def noise(h=61, w=97, seed=7):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def blobs(h=90, w=140, seed=11):
    """smooth random texture: well separated maxima of very different strengths"""
    rng = np.random.default_rng(seed)
    img = rng.normal(0, 1, (h, w))
    for _ in range(3):
        img = (img + np.roll(img, 1, 0) + np.roll(img, -1, 0) + np.roll(img, 1, 1) + np.roll(img, -1, 1)) / 5
    img = (img - img.min()) / (img.max() - img.min())
    return np.rint(255 * img).astype(np.uint8)


def test_bright_rectangle():
    corners, full = G.good_features_to_track(rectangle(), 0, 0.01, 8, full=True)
    assert len(full["indices"]) == 4 and corners.shape == (4, 2) and corners.dtype == np.float32
    want = {(20, 16), (43, 16), (20, 31), (43, 31)}  # the corner pixels of [16:32, 20:44]
    hit = set()
    for x, y in corners:
        near = [c for c in want if abs(c[0] - x) <= 1 and abs(c[1] - y) <= 1]
        assert len(near) == 1, (x, y)
        hit.add(near[0])
    assert hit == want


def test_flat_image_has_no_corner():
    for v in (0, 93, 255):
        corners, full = G.good_features_to_track(np.full((48, 64), v, np.uint8), 0, 0.01, 8, full=True)
        assert corners.shape == (0, 2) and len(full["indices"]) == 0 and not full["eig"].any()


def test_non_positive_response_is_never_a_corner():
    """a horizontal ramp: one gradient direction only, the smaller eigenvalue is 0 (or rounds below it) everywhere"""
    img = np.tile(np.arange(0, 192, 2, dtype=np.uint8), (40, 1))
    eig = G.corner_min_eigen_val(img)
    assert eig.max() <= 0
    assert len(G.good_features_to_track(img, 0, 0.01, 0)) == 0
    # and beside real corners: nothing at or below zero survives the threshold
    corners, full = G.good_features_to_track(np.hstack([img, rectangle()[:40]]), 0, 1e-9, 0, full=True)
    assert len(corners) and np.all(full["values"] > 0)


def test_checkerboard_ties_go_by_index_descending():
    corners, full = G.good_features_to_track(checkerboard(), 0, 0.01, 8, full=True)
    val, idx = full["values"], full["indices"]
    # 11 x 7 crossings of four pixels each share ONE value (the box sums of all of them are permutations of
    # (1920000, 0, 1920000)); the other 14 candidates, beside the last column, are weaker
    assert len(idx) == 322 and len(corners) == 77
    assert np.all(np.diff(val.astype(np.float64)) <= 0)
    top = val == val[0]
    assert top.sum() == 308 and np.all(top[:308])
    for v in np.unique(val):
        assert np.all(np.diff(idx[val == v]) < 0), v  # equal values: row-major index descending
    assert idx[0] == idx.max() or val[0] > val[-1]
    # the first corner is the tied candidate with the largest index
    w = 97
    assert (corners[0, 0], corners[0, 1]) == (idx[0] % w, idx[0] // w) and idx[0] == idx[top].max()


def grid_select(idx, w, h, max_corners, min_distance):
    """Rule 5 with OpenCV's cell grid, cell = cvRound(minDistance) (np.rint: half to even), 3 x 3 cells searched"""
    n = len(idx)
    limit = max_corners if max_corners > 0 else n
    if min_distance < 1:
        return np.arange(min(n, limit))
    cell = int(np.rint(min_distance))
    d2 = np.float32(np.float64(min_distance) * np.float64(min_distance))
    grid = {}
    kept = []
    for i in range(n):
        x, y = int(idx[i] % w), int(idx[i] // w)
        cx, cy = x // cell, y // cell
        good = True
        for yy in range(cy - 1, cy + 2):
            for xx in range(cx - 1, cx + 2):
                for (px, py) in grid.get((xx, yy), ()):
                    if np.float32((x - px) ** 2 + (y - py) ** 2) < d2:
                        good = False
        if good:
            grid.setdefault((cx, cy), []).append((x, y))
            assert len(grid[(cx, cy)]) <= (1 if cell == 1 else 4)  # the occupancy bound the kernel relies on
            kept.append(i)
            if len(kept) == limit:
                break
    return np.array(kept, np.int64)


DISTANCES = [0.0, 0.99, 1.0, 1.4, 1.5, 2.0, 2.5, 3.5, 8.0, 8.5, 12.5, 40.0]


@pytest.mark.parametrize("name", ["noise", "blobs", "checkerboard"])
def test_greedy_properties_and_grid_variant(name):
    img = {"noise": noise(), "blobs": blobs(), "checkerboard": checkerboard()}[name]
    h, w = img.shape
    val, idx = G.candidates(G.corner_min_eigen_val(img), 0.01)
    assert len(idx) > 100
    xs, ys = idx % w, idx // w
    for d in DISTANCES:
        for limit in (0, 17):
            kept = G.select(idx, w, limit, d)
            assert np.array_equal(kept, grid_select(idx, w, h, limit, d)), (d, limit)
            assert np.all(np.diff(kept) > 0)                       # in the order of rule 4 ...
            assert np.all(np.diff(val[kept].astype(np.float64)) <= 0)  # ... so the responses do not increase
            if limit:
                assert len(kept) <= limit
            if d < 1:
                assert np.array_equal(kept, np.arange(len(idx) if not limit else min(limit, len(idx))))
                continue
            d2 = np.float64(np.float32(d * d))
            kx, ky = xs[kept], ys[kept]
            dist2 = (kx[:, None] - kx[None, :]) ** 2 + (ky[:, None] - ky[None, :]) ** 2
            np.fill_diagonal(dist2, 1 << 40)
            assert dist2.min() >= d2, d                            # every accepted pair is at least d apart
            # every rejected candidate (up to the last accepted one) has an EARLIER accepted corner closer than d
            is_kept = np.zeros(len(idx), bool)
            is_kept[kept] = True
            for i in np.flatnonzero(~is_kept[:kept[-1] + 1]):
                earlier = kept[kept < i]
                assert np.any((xs[i] - xs[earlier]) ** 2 + (ys[i] - ys[earlier]) ** 2 < d2), (d, i)
            if not limit:  # without a limit the same holds to the end of the list
                for i in np.flatnonzero(~is_kept):
                    assert np.any((xs[i] - kx) ** 2 + (ys[i] - ky) ** 2 < d2), (d, i)


def test_rule_1_against_float64():
    """The float32 sequence of rule 1 against the same formula in float64 on the same integers.

    With u = 2^-24, A = a + c and r = sqrt((a - c)^2 + b^2) <= A (exact values, from the exact constants):
      a, b, c   two roundings each (the constant K, the product): relative error 2u
      a + c     3u A
      d = a - c absolute error 2u A + u |d|
      t, r      d -> r is 1-Lipschitz, as is b -> r: 2u A + u |d| + 2u |b|; the roundings of d * d, b * b, their sum
                (together 2u relative on t, u on r) and of the square root (u): 2u r; with |d|, |b| <= r <= A: 7u A
      e         3u A + 7u A + u |e| <= 11u A
    to first order; 12u A covers the second-order terms."""
    u = 2.0 ** -24
    worst = 0.0
    for img in (noise(), blobs(), checkerboard(), rectangle(), noise(50, 70, seed=1) // 16):
        sxx, sxy, syy = G.structure_sums(img)
        assert max(sxx.max(), syy.max(), abs(sxy).max()) < 2 ** 24  # exact in float32
        e32 = G.min_eig_f32(sxx, sxy, syy)
        s2 = 1.0 / (3060.0 * 3060.0)
        a, b, c = 0.5 * s2 * sxx, s2 * sxy.astype(np.float64), 0.5 * s2 * syy
        e64 = (a + c) - np.sqrt((a - c) ** 2 + b * b)
        bound = 12 * u * (a + c)
        diff = np.abs(e32.astype(np.float64) - e64)
        assert np.all(diff <= bound), float((diff - bound).max())
        nz = bound > 0
        worst = max(worst, float((diff[nz] / bound[nz]).max()))
    print("rule 1: worst |e32 - e64| / bound = %.3f" % worst)
    assert worst > 0  # the comparison is not vacuous


def test_threshold_and_quality_level():
    img = noise()
    eig = G.corner_min_eigen_val(img)
    v1, i1 = G.candidates(eig, 1.0)  # e > max never holds
    assert len(i1) == 0
    lo, _ = G.candidates(eig, 0.001)
    hi, _ = G.candidates(eig, 0.3)
    thr = np.float32(np.float64(eig.max()) * 0.3)
    assert len(hi) < len(lo) and np.all(hi > thr) and np.all(lo[len(hi):] <= thr) and np.array_equal(lo[:len(hi)], hi)


def test_border_pixels_are_no_candidates():
    img = noise(30, 40, seed=5)
    _, idx = G.candidates(G.corner_min_eigen_val(img), 0.0001)
    x, y = idx % 40, idx // 40
    assert len(idx) > 20 and x.min() >= 1 and x.max() <= 38 and y.min() >= 1 and y.max() <= 28
