"""CPU-only, the oracle alone: rule C's radius R = max(patch_size / 2, 20) is sufficient.  For
points exactly R from each border of the 320 x 160 crop of smoke(), in the corners and along the edges, and a few
thousand angles given explicitly to the oracle's BRIEF, no test is skipped (nskip == 0) and no box sum reaches outside
the image (noob == 0): all 256 bits of an ORBX_PD_OK slot are pinned.  The orientation patch lies inside the image too.
One pixel closer to a border the guarantee is gone, so R is not larger than it has to be for the pattern."""
import numpy as np
import pytest

import oracle_lib as O
import reassoc_ref as R

W, H = 320, 160


@pytest.fixture(scope="module")
def crop():
    return O.load_kitti(0)[100:260, 300:620].copy()


def border_points(r):
    xs, ys = [r, 97, W // 2, W - 1 - r], [r, 61, H - 1 - r]
    pts = [(x, y) for x in xs for y in (r, H - 1 - r)] + [(x, y) for x in (r, W - 1 - r) for y in ys]
    return np.array(sorted(set(pts)), np.int32)


def angles():
    a = np.linspace(-np.pi, np.pi, 4001).astype(np.float32)  # what atan2f returns, both ends included
    return np.concatenate([a, np.float32([0.0, np.pi / 4, -np.pi / 4, np.pi / 2, 3 * np.pi / 4])])


@pytest.mark.parametrize("patch_size", [31, 41, 9])
def test_r_from_every_border_is_enough(crop, patch_size):
    r = R.pd_radius(patch_size)
    assert r == max(patch_size // 2, 20)
    pts, ang = border_points(r), angles()
    assert len(pts) >= 10 and {tuple(p) for p in pts} >= {(r, r), (W - 1 - r, r), (r, H - 1 - r), (W - 1 - r, H - 1 - r)}
    for p in pts:
        _, valid, nskip, noob = O.brief(crop, np.tile(p, (len(ang), 1)), ang)
        assert nskip == 0 and noob == 0, (tuple(p), nskip, noob)
        assert (valid == 0xff).all()
        pr = patch_size // 2  # the orientation patch (src/orb_cpu.cpp:152-156)
        assert p[0] - pr >= 0 and p[0] + pr <= W - 1 and p[1] - pr >= 0 and p[1] + pr <= H - 1


def test_the_pattern_reaches_18(crop):
    """the largest rotated and rounded offset over these angles is 18: with the 5x5 box's 2 that is rule C's 20"""
    ang = angles()
    # a point 19 from the left border: some angle sends a box to x = 19 - 18 - 2 < 0 ... which the reference's own
    # bounds rule skips (cx < 2), so the bit is not pinned there
    _, _, nskip, noob = O.brief(crop, np.tile(np.int32([19, 80]), (len(ang), 1)), ang)
    assert nskip > 0
    # ... and at 20 nothing is skipped (the parametrised test), so 18 is reached and 19 is not
    _, _, nskip, noob = O.brief(crop, np.tile(np.int32([20, 80]), (len(ang), 1)), ang)
    assert nskip == 0 and noob == 0


def test_describe_points_reference_states(crop):
    """rules A-C of the numpy restatement on a handful of points"""
    p = O.gpu_params(blur_levels=0)
    pts = np.float32([[20.5, 20.0], [21.5, 20.0], [19.49, 80], [299.0, 139.0], [299.5, 139.0], [300.0, 100.0],
                      [np.nan, 5], [np.inf, 5], [-0.0, 0.0], [-1.0, 5], [319.0, 159.0], [319.01, 100.0], [50, 50]])
    got = R.describe_points(crop, pts, p, seen=np.r_[np.ones(12, np.int32), 0], seen_min=1)
    S = [R.PD_OK, R.PD_OK, R.PD_BORDER, R.PD_OK, R.PD_BORDER, R.PD_BORDER, R.PD_NONE, R.PD_NONE, R.PD_BORDER,
         R.PD_NONE, R.PD_BORDER, R.PD_NONE, R.PD_NONE]
    assert got["state"].tolist() == S
    assert got["pix"][:2].tolist() == [[20, 20], [22, 20]] and got["pix"][4].tolist() == [300, 139]  # ties to even
    assert got["n_ok"] == 3 and got["nskip"] == 0 and got["noob"] == 0
    assert not got["desc"][got["state"] != R.PD_OK].any() and not got["angle"][got["state"] != R.PD_OK].any()
    assert got["desc"][got["state"] == R.PD_OK].any(axis=1).all()
    assert R.describe_points(crop, pts, p, count=1)["state"].tolist() == [R.PD_OK] + [R.PD_NONE] * 12
