"""Harris windows no other test reaches: 1, 9, 11, 13 and 15 (validate_params and orbx_harris accept every odd window
up to 15; 3, 5 and 7 run the packed 16-bit path, the others k_level_select<0> and the generic paths of k_lvl_harris
and k_harris2_flat).  These are the windows whose (K + 2)^2 neighbourhood leaves the image by more than one row or
column at a FAST keypoint 3 px from the border.

CPU (no GPU): the oracle's Harris against the numpy restatement of test_oracle_vs_numpy.py, bit for bit, and against
a float64 evaluation of the same weighted sums, within a bound derived from the oracle's own float roundings.
GPU: ctx.harris against the oracle bit for bit on the same points and images (border and interior points mixed in
one call), and the whole path at windows 1, 9 and 15: a single frame, a batch of 2 (a workgroup per (level, frame)),
a batch of 256 (a workgroup per frame) and the spread kernels (nfeatures = 1000: caps above 512), on 320 x 160 frames
and on 96 x 20 frames whose fourth level is 9 rows high: an 11-row neighbourhood reflects on both sides there."""
import concurrent.futures as cf
import importlib.util
import os

import numpy as np
import pytest

import oracle_lib as O
import test_oracle_vs_numpy as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(ROOT, "tools", "fuzz_parity.py"))
F = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(F)

WINDOWS = [1, 9, 11, 13, 15]
U = 2.0 ** -24  # unit roundoff of float32


def image(name):
    w, h = {"noise": (320, 160), "8x8": (8, 8), "9x17": (9, 17), "17x9": (17, 9)}[name]
    return np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w), dtype=np.uint8)


def points(w, h):
    """interior points, points 3 px from each border and each corner, (0, 0) and (w - 1, h - 1) -- mixed, so that one
    call holds border and interior points side by side"""
    rng = np.random.default_rng(w + h)
    xs, ys = [3, w // 2, w - 4], [3, h // 2, h - 4]
    pts = [(x, y) for y in ys for x in xs]  # the four corners, the four borders and the centre
    pts += [(0, 0), (w - 1, h - 1), (0, h - 1), (w - 1, 0)]
    if w > 40:
        for _ in range(24):  # interior: at least 10 px from every border; and more border points
            pts.append((int(rng.integers(10, w - 10)), int(rng.integers(10, h - 10))))
            pts.append((int(rng.integers(3, w - 3)), int(rng.choice([3, h - 4]))))
            pts.append((int(rng.choice([3, w - 4])), int(rng.integers(3, h - 3))))
    order = rng.permutation(len(pts))
    return np.array(pts, np.int32)[order]


def harris_f64(img, kps, K, kk):
    """the sums of oracle_harris in float64: exact integer Sobel sums at REFLECT_101 coordinates of the product image,
    the oracle's own float32 Gaussian weights.  Returns the response and |AC| + B^2 + k (A + C)^2."""
    h, w = img.shape
    p = img.astype(np.int64)[N.np_reflect(h, 1)][:, N.np_reflect(w, 1)]
    gx = (p[0:h, 2:] + 2 * p[1:h + 1, 2:] + p[2:, 2:]) - (p[0:h, 0:w] + 2 * p[1:h + 1, 0:w] + p[2:, 0:w])
    gy = (p[2:, 0:w] + 2 * p[2:, 1:w + 1] + p[2:, 2:]) - (p[0:h, 0:w] + 2 * p[0:h, 1:w + 1] + p[0:h, 2:])
    g = O.gaussian_kernel(K).astype(np.float64)
    r = K // 2
    ry, rx = N.np_reflect(h, r), N.np_reflect(w, r)
    k64 = float(np.float32(kk))
    out, size = [], []
    for x, y in kps:
        yy, xx = ry[y:y + K], rx[x:x + K]
        wx, wy = gx[np.ix_(yy, xx)].astype(np.float64), gy[np.ix_(yy, xx)].astype(np.float64)
        A, B, C = float((wx * wx * g).sum()), float((wx * wy * g).sum()), float((wy * wy * g).sum())
        out.append((A * C - B * B) - k64 * (A + C) * (A + C))
        size.append(abs(A * C) + B * B + k64 * (A + C) * (A + C))
    return np.array(out), np.array(size)


@pytest.mark.parametrize("name", ["noise", "8x8", "9x17", "17x9"])
@pytest.mark.parametrize("K", WINDOWS)
def test_oracle_equals_the_numpy_restatement(K, name):
    img = image(name)
    pts = points(img.shape[1], img.shape[0])
    for kk in (0.04, 0.0):
        ref = O.harris(img, pts, K, kk)
        got = N.np_harris(img, pts, K, kk)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (K, name, kk)


@pytest.mark.parametrize("name", ["noise", "8x8", "9x17", "17x9"])
@pytest.mark.parametrize("K", WINDOWS)
def test_oracle_against_float64(K, name):
    """Roundings of oracle_harris (harris_at), u = 2^-24.  Each of A, B, C is a sum of K^2 terms; a term costs at most
    three roundings (the product of the gradients -- exact in fact, |gx gy| <= 1020^2 < 2^24 --, the product with the
    weight, the addition), each at most u times the running sum of absolute values, which never exceeds the final
    one: |dA| <= e A, |dC| <= e C, |dB| <= e sum|w gx gy| <= e sqrt(AC) (Cauchy-Schwarz), with e = 3 K^2 u / (1 - 3 K^2 u).
    Closing products, first order:  a c: (2 e + u) AC;  b b: 2 |B| e sqrt(AC) + u B^2 <= e (AC + B^2) + u B^2;
    the difference: u (AC + B^2);  k (a + c) (a + c): the sum e + u, two factors of it and two products:
    (2 e + 4 u) k (A + C)^2;  the last difference u (AC + B^2 + k (A + C)^2).  Every coefficient is at most
    3 e + 5 u, so  |R_oracle - R_64| <= (3 e + 5 u) (|AC| + B^2 + k (A + C)^2), with 1 % for the second-order terms."""
    img = image(name)
    pts = points(img.shape[1], img.shape[0])
    e = 3 * K * K * U / (1 - 3 * K * K * U)
    for kk in (0.04, 0.06, 0.0):
        ref = O.harris(img, pts, K, kk).astype(np.float64)
        r64, size = harris_f64(img, pts, K, kk)
        ratio = np.abs(ref - r64) / np.maximum(size * U, 1e-300)
        print("K %d %s k %.2f: largest error %.2f u, bound %.0f u" % (K, name, kk, ratio.max(), 1.01 * (3 * e + 5 * U) / U))
        assert np.all(np.abs(ref - r64) <= 1.01 * (3 * e + 5 * U) * size), (K, name, kk, ratio.max())
        assert size.max() > 0


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_harris_operator_equals_the_oracle(pkg):
    p = pkg.default_params("gpu", max_width=320, max_height=160)
    with pkg.Context(p) as ctx:
        for name in ("noise", "8x8", "9x17", "17x9"):
            img = image(name)
            pts = points(img.shape[1], img.shape[0])
            for K in WINDOWS + [3, 5, 7]:
                for kk in (0.04, 0.0):
                    ref = O.harris(img, pts, K, kk)
                    got = ctx.harris(img, pts, K, kk)
                    bad = np.nonzero(got.view(np.uint32) != ref.view(np.uint32))[0]
                    assert len(bad) == 0, (name, K, kk, pts[bad][:8], got[bad][:8], ref[bad][:8])


BASE = dict(nlevels=4, threshold=20, n=9, nms_window=3, patch_size=31, harris_k=0.04, blur_levels=2, blur_kind=0)
SHAPES = {
    # name: frame size, scale factor, nfeatures
    "320x160": (320, 160, 1.2, 200),
    "96x20": (96, 20, 1.3, 240),       # level heights 20, 15, 12, 9
    "spread": (320, 160, 1.2, 1000),   # caps above 512: k_lvl_compact, k_lvl_harris, k_lvl_rank
}
_refs = {}


def frames_and_refs(shape, K):
    """four frames of the shape and the oracle's results for them (computed once)"""
    if (shape, K) not in _refs:
        w, h, sf, nf = SHAPES[shape]
        kw = dict(BASE, nfeatures=nf, scale_factor=sf, harris_window=K)
        rng = np.random.default_rng(w + K)
        fr = []
        for cell in (3, 4, 5, 6):  # random cells of 40 / 220 (dense corners on every level) under a little noise
            cells = np.kron(rng.integers(0, 2, (h // cell + 1, w // cell + 1)), np.ones((cell, cell), np.int64))[:h, :w]
            fr.append((40 + 180 * cells + rng.integers(-10, 11, (h, w))).astype(np.uint8))
        fr = np.stack(fr)
        O.lib()
        with cf.ThreadPoolExecutor(4) as ex:  # ctypes releases the GIL
            refs = list(ex.map(lambda f: O.detect_and_compute_gpu(f, O.gpu_params(**kw)), fr))
        _refs[(shape, K)] = (kw, fr, refs)
    return _refs[(shape, K)]


def check_batch(r, refs, n, tag):
    for i in range(n):
        m = int(r["counts"][i])
        got = dict(count=m, **{k: r[k][i, :m] for k in ("kps", "kps_level", "levels", "angles", "responses", "desc")})
        F.check(got, refs[i % len(refs)], (tag, i))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("K", [1, 9, 15])
def test_whole_path(pkg, K, shape):
    w, h, sf, nf = SHAPES[shape]
    kw, fr, refs = frames_and_refs(shape, K)
    if shape == "96x20":
        # what the shape is for: keypoints of the 9-row level whose K + 2 rows leave the image above AND below
        _, hl = O.level_size(w, h, sf, 3)
        reach = (K + 2) // 2
        y = np.concatenate([r["kps_level"][r["levels"] == 3][:, 1] for r in refs])
        assert hl == 9 and len(y) > 0
        assert K < 9 or ((y - reach < 0) & (y + reach > hl - 1)).any(), (hl, y)
    if shape == "spread":
        assert 2 * O.level_quota(nf, sf, 4, 0) > 512
    # every frame has keypoints on the top level too
    assert all((r["levels"] == 3).any() and (r["levels"] == 0).any() for r in refs)
    for n in (1, 2, 256):
        p = pkg.default_params("gpu", max_width=w, max_height=h, max_batch=n, **kw)
        with pkg.Context(p) as c:
            cap = max(c.plan(w, h)["out_capacity"], 1)
            if n == 1:
                for i in range(2):
                    F.check(c.detect_and_compute(fr[i]), refs[i], (shape, K, "single", i))
                continue
            c.batch_host(fr[np.arange(n) % len(fr)])
            check_batch(c.batch_fetch(0, n, cap), refs, n, (shape, K, n))
