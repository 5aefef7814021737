"""Numpy restatement of the library's Shi-Tomasi corner detection (rules 1-6): what
orbx_corner_min_eigen_val and orbx_good_features_to_track compute, bit for bit.  Independent of the kernels: whole-array
numpy operations, one float32 rounding per documented operation (numpy evaluates each ufunc on its own: no
contraction), and a brute-force O(n^2) greedy selection without any cell grid.

cv::goodFeaturesToTrack(image, corners, maxCorners, qualityLevel, minDistance) with no mask, blockSize 3,
gradientSize 3, useHarrisDetector false."""
import numpy as np

K = np.float32(1.0 / 9363600.0)  # s^2, s = 1 / (4 * 3 * 255): OpenCV's scale for CV_8U, aperture 3, block 3
KH = np.float32(0.5) * K         # exact


def _pad(a):
    return np.pad(a, 1, mode="reflect")  # numpy's "reflect" is REFLECT_101


def _box3(m):
    q = _pad(m)
    h, w = m.shape
    return sum(q[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))


def structure_sums(img):
    """Rule 1, the integer part: (Sxx, Sxy, Syy), int64, each the 3x3 box sum of a REFLECT_101-extended PRODUCT map
    of the 3x3 Sobel derivatives of the REFLECT_101-extended image."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    p = _pad(img.astype(np.int64))
    gx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    gy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    return _box3(gx * gx), _box3(gx * gy), _box3(gy * gy)


def min_eig_f32(sxx, sxy, syy):
    """Rule 1, the float32 sequence: a = KH * Sxx, b = K * Sxy, c = KH * Syy, d = a - c, t = d * d + b * b,
    e = (a + c) - sqrt(t)."""
    a = KH * sxx.astype(np.float32)
    b = K * sxy.astype(np.float32)
    c = KH * syy.astype(np.float32)
    d = a - c
    t = d * d + b * b
    e = (a + c) - np.sqrt(t)
    assert e.dtype == np.float32
    return e


def corner_min_eigen_val(img):
    return min_eig_f32(*structure_sums(img))


def candidates(eig, quality_level):
    """Rules 2-4: (values float32, row-major indices int64) of the candidates in selection order."""
    h, w = eig.shape
    mx = eig.max()
    if not mx > 0:
        return np.zeros(0, np.float32), np.zeros(0, np.int64)
    thr = np.float32(np.float64(mx) * np.float64(quality_level))
    t = np.where(eig > thr, eig, np.float32(0))  # THRESH_TOZERO: what is not above thr (all of e <= 0) is 0
    q = np.pad(t, 1, mode="constant", constant_values=0)  # outside the image: ignored (t >= 0)
    dil = np.max([q[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], axis=0)
    cand = (t != 0) & (t == dil)
    cand[0, :] = cand[-1, :] = False
    cand[:, 0] = cand[:, -1] = False
    idx = np.flatnonzero(cand.reshape(-1))
    val = t.reshape(-1)[idx]
    order = np.lexsort((idx, val))[::-1]  # value descending, equal values: index descending
    return val[order], idx[order]


def select(idx, w, max_corners, min_distance):
    """Rule 5, brute force: positions (into idx) of the accepted candidates, in order."""
    n = len(idx)
    limit = max_corners if max_corners > 0 else n
    if min_distance < 1:
        return np.arange(min(n, limit))
    d2 = np.float32(np.float64(min_distance) * np.float64(min_distance))
    xs, ys = idx % w, idx // w
    ax, ay = np.zeros(n, np.int64), np.zeros(n, np.int64)
    kept = []
    for i in range(n):
        m = len(kept)
        dx, dy = xs[i] - ax[:m], ys[i] - ay[:m]
        # the exact integer, rounded to float32 once, against (float)(d * d)
        if m and np.any((dx * dx + dy * dy).astype(np.float32) < d2):
            continue
        ax[m], ay[m] = xs[i], ys[i]
        kept.append(i)
        if len(kept) == limit:
            break
    return np.array(kept, np.int64)


def good_features_to_track(img, max_corners, quality_level, min_distance, full=False):
    """Rules 1-6: (n, 2) float32 corners (x, y) in acceptance order.  full: also the dict of intermediate results."""
    eig = corner_min_eigen_val(img)
    val, idx = candidates(eig, quality_level)
    w = eig.shape[1]
    kept = select(idx, w, max_corners, min_distance)
    k = idx[kept]
    corners = np.stack([(k % w).astype(np.float32), (k // w).astype(np.float32)], axis=1).reshape(-1, 2)
    if full:
        return corners, dict(eig=eig, values=val, indices=idx, kept=kept)
    return corners
