"""Border keypoints through the throughput instantiation of the batched describe kernel (k_describe2<4, 4, 6>),
through the batch C ABI against the oracle, bit for bit.

tests/test_select_describe_edges.py keeps out_capacity x frames <= 8192 and so only reaches the
one-keypoint-per-wave instantiation.  The batches here exceed that threshold (asserted in every case), on shapes
whose levels exercise each way a 41 x 48 neighbourhood can leave a level:

  64 x 192   level 0 has w == pitch (no padding to absorb a read past a row's end); the top level is 37 rows
             high, so a neighbourhood overruns above and below at once
  150 x 230  level 1 is 192 wide (no padding again), the other levels have padding
  96 x 256   level 0 has w == pitch, levels 1 and 2 (213 and 178 wide) have padding

Each case first counts, from the oracle's output, the keypoints within 20 px of each of the four sides of every
level and asserts every count is positive, so it cannot pass by having no border keypoints.
"""
import functools

import numpy as np
import pytest

import test_select_describe_edges as E

pytestmark = pytest.mark.gpu

MARGIN = 20  # the describe kernel's neighbourhood radius: closer to a side than this, a keypoint is a border one
KW = dict(E.BASE, blur_levels=2, patch_size=31, harris_window=7)
SHAPES = {  # (h, w): frames, nfeatures, nlevels
    (64, 192): (12, 800, 4),
    (150, 230): (12, 800, 4),
    (96, 256): (16, 600, 3),
}


def shape_kw(shape, **over):
    _, nfeatures, nlevels = SHAPES[shape]
    return dict(KW, nfeatures=nfeatures, nlevels=nlevels, **over)


@functools.lru_cache(maxsize=None)
def images(shape):
    h, w = shape
    imgs = np.stack([E.edge_image(1000 + k, h, w) for k in range(SHAPES[shape][0])])
    imgs.setflags(write=False)
    return imgs


@functools.lru_cache(maxsize=None)
def references(shape, patch_size=31):
    """the oracle's result for every frame of the shape: computed once, shared by the cases"""
    kw = shape_kw(shape, patch_size=patch_size)
    return tuple(E.reference(img, kw, 0) for img in images(shape))


def side_counts(refs, level_w, level_h, nlevels):
    """keypoints within MARGIN px of the left, right, top and bottom side, per level, over all frames"""
    n = np.zeros((nlevels, 4), np.int64)
    both = 0
    for ref in refs:
        x, y, lv = ref["kps_level"][:, 0], ref["kps_level"][:, 1], ref["levels"]
        w, h = level_w[lv], level_h[lv]
        sides = (x < MARGIN, x >= w - MARGIN, y < MARGIN, y >= h - MARGIN)
        for s, m in enumerate(sides):
            n[:, s] += np.bincount(lv[m], minlength=nlevels)[:nlevels]
        both += int((sides[2] & sides[3]).sum())
    return n, both


def run(pkg, shape, frames=None, host=False, patch_size=31, throughput=True):
    h, w = shape
    imgs = images(shape)[:frames]
    refs = references(shape, patch_size)[:len(imgs)]
    B = len(imgs)
    kw = shape_kw(shape, patch_size=patch_size)
    p = pkg.default_params("gpu", max_width=w, max_height=h, max_batch=B, select_mode=0, **kw)
    with pkg.Context(p) as c:
        plan = c.plan(w, h)
        cap = plan["out_capacity"]
        # above 8192 output slots the batch runs k_describe2<4, 4, 6>, up to it k_describe2<1, 4, 1>
        assert (cap * B > 8192) == throughput, (cap, B)
        n, both = side_counts(refs, plan["level_w"], plan["level_h"], kw["nlevels"])
        assert (n > 0).all(), n
        c.set_host_results(host)
        c.batch_host(np.ascontiguousarray(imgs))
        hv = E.F.host_record(c) if host else None
        r = c.batch_fetch(0, B, cap)
    for i, ref in enumerate(refs):
        k = int(r["counts"][i])
        got = dict(count=k, kps=r["kps"][i, :k], kps_level=r["kps_level"][i, :k], levels=r["levels"][i, :k],
                   angles=r["angles"][i, :k], responses=r["responses"][i, :k], desc=r["desc"][i, :k])
        E.F.check(got, ref, (shape, i, patch_size))
        if hv is not None:  # the pinned record the kernel wrote itself
            assert int(hv["counts"][i]) == k
            assert np.array_equal(hv["kps16"][i, :k].astype(np.int32), r["kps"][i, :k])
            assert np.array_equal(hv["angles"][i, :k].view(np.uint32), r["angles"][i, :k].view(np.uint32))
            assert np.array_equal(hv["desc"][i, :k], r["desc"][i, :k])
    return n, both


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_border_keypoints_throughput_kernel(pkg, shape):
    n, both = run(pkg, shape)
    if shape == (64, 192):  # the 37-row top level: neighbourhoods that overrun above and below at once
        assert both > 0


def test_border_keypoints_host_record(pkg):
    run(pkg, (64, 192), host=True)


def test_border_keypoints_window_equals_fetch_radius(pkg):
    """patch_size 41: the orientation window is the whole fetched neighbourhood"""
    run(pkg, (150, 230), patch_size=41)


def test_border_keypoints_single_keypoint_waves(pkg):
    """control: the same images, three frames, on the one-keypoint-per-wave instantiation"""
    run(pkg, (64, 192), frames=3, throughput=False)
