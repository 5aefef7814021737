"""The orientation moments of the batched describe kernel (k_describe2) with the compile-time window of
patch_size 31 (rows and columns 5 ... 35 of the 41-row neighbourhood, S carried above the row-weighted sum in one
multiply-add chain), against the oracle: angles bit for bit (the issue asks for 1e-4), descriptors bit for bit.
patch_size 29 and 33 run the run-time window on the same frames.

Frames of 160 x 120, built so that the cases are there by construction (checked on the CPU, with the oracle, in
test_frames_hold_the_cases):

  dots    all 255 with a few dark dots: the largest S and M the packing can meet.  Every keypoint dot has a mark
          in row 5 or row 35 of its neighbourhood (15 rows above / below: the window's first and last row) and one
          in row 1 or 39 (outside, and out of the blur's reach of it), so a window that is a row off changes the
          angle; the dots cover every x mod 4, the four byte offsets `off` of a patch in its first dword.
  border  mild noise with dark blobs centred exactly 15 and 14 pixels from each side: the window just inside the
          level, and just outside, where the angle is 0.
  noise   two frames of uniform noise (some 600 keypoints each).

Each case runs the frames through the one-keypoint-per-wave instantiation (a small batch) and, repeated, through the
four-keypoint one (more than 8192 output slots).
"""
import functools

import numpy as np
import pytest

import test_select_describe_edges as E

H, W = 120, 160
KW = dict(E.BASE, nfeatures=600, nlevels=3, blur_levels=2)
PATCH_SIZES = (31, 29, 33)
# level-0 positions (x, y) of the dots frame's keypoint dots: x covers every residue mod 4, and no dot or mark of one
# lies in the window of another
DOTS = [(24, 35), (61, 35), (98, 35), (135, 35), (24, 85), (61, 85), (98, 85), (135, 85)]
# ... and of the border frame's dots: 15 px from a side (window inside), 14 px (outside: angle 0)
NEAR = [(15, 40), (W - 16, 50), (60, 15), (70, H - 16)]
OUT = [(14, 70), (W - 15, 80), (100, 14), (110, H - 15)]


def dots_frame():
    img = np.full((H, W), 255, np.uint8)
    for i, (x, y) in enumerate(DOTS):
        img[y, x] = 0
        up = i % 2 == 0
        img[y - 15 if up else y + 15, x + 2] = 0  # row 5 / 35 of the neighbourhood: inside the window
        # ... and outside it, beyond the reach of the 5 x 5 blur (the window's own mark spreads over rows 33 ... 37 or
        # 3 ... 7, across the window's edge: a window one row off changes the angle)
        img[y + 19 if up else y - 19, x - 6] = 0  # row 39 / 1
    return img


def noise_frame(seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W)).astype(np.uint8)


def border_frame():
    """3 x 3 dark blobs (a single pixel does not survive the blur as a corner) on mild noise"""
    rng = np.random.default_rng(7)
    img = np.clip(np.rint(150.0 + 20.0 * rng.standard_normal((H, W))), 0, 255).astype(np.uint8)
    for x, y in NEAR + OUT:
        img[y - 1:y + 2, x - 1:x + 2] = 0
    return img


@functools.lru_cache(maxsize=None)
def frames():
    imgs = np.stack([dots_frame(), border_frame(), noise_frame(11), noise_frame(12)])
    imgs.setflags(write=False)
    return imgs


@functools.lru_cache(maxsize=None)
def references(patch_size):
    """the oracle's result per frame: computed once, shared by the cases"""
    return tuple(E.reference(img, dict(KW, patch_size=patch_size), 0) for img in frames())


def level0(ref):
    """{(x, y): angle} of the level-0 keypoints"""
    m = ref["levels"] == 0
    return {(int(x), int(y)): float(a) for (x, y), a in zip(ref["kps_level"][m], ref["angles"][m])}


def test_frames_hold_the_cases(oracle):
    dots, border, n1, n2 = references(31)
    kp = level0(dots)
    for x, y in DOTS:
        assert (x, y) in kp and kp[(x, y)] != 0.0, (x, y)
    assert {x % 4 for x, _ in DOTS} == {0, 1, 2, 3}
    # the window's marks count and the ones outside do not: the angle is the one of a frame without the outer marks
    clean = dots_frame()
    for i, (x, y) in enumerate(DOTS):
        clean[y + 19 if i % 2 == 0 else y - 19, x - 6] = 255
    kc = level0(E.reference(clean, dict(KW, patch_size=31), 0))
    for x, y in DOTS:
        assert kc[(x, y)] == kp[(x, y)], (x, y)
    kb = level0(border)
    for x, y in NEAR:
        assert (x, y) in kb and kb[(x, y)] != 0.0, (x, y)
    for x, y in OUT:
        assert (x, y) in kb and kb[(x, y)] == 0.0, (x, y)
    for ref in (n1, n2):
        assert len(ref["kps"]) > 100


def run(pkg, patch_size, repeat):
    imgs = np.ascontiguousarray(np.tile(frames(), (repeat, 1, 1)))
    refs = references(patch_size) * repeat
    B = len(imgs)
    p = pkg.default_params("gpu", max_width=W, max_height=H, max_batch=B, select_mode=0, **dict(KW, patch_size=patch_size))
    with pkg.Context(p) as c:
        cap = c.plan(W, H)["out_capacity"]
        # above 8192 output slots a batch runs four keypoints per wave, up to it one
        assert (cap * B > 8192) == (repeat > 1), (cap, B)
        c.batch_host(imgs)
        r = c.batch_fetch(0, B, cap)
    for i, ref in enumerate(refs):
        k = int(r["counts"][i])
        got = dict(count=k, kps=r["kps"][i, :k], kps_level=r["kps_level"][i, :k], levels=r["levels"][i, :k],
                   angles=r["angles"][i, :k], responses=r["responses"][i, :k], desc=r["desc"][i, :k])
        E.F.check(got, ref, (patch_size, repeat, i))  # (angles and descriptors bit for bit)
        assert np.allclose(got["angles"], ref["angles"], atol=1e-4), (patch_size, i)


@pytest.mark.gpu
@pytest.mark.parametrize("patch_size", PATCH_SIZES)
def test_moments_one_keypoint_per_wave(pkg, patch_size):
    run(pkg, patch_size, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("patch_size", PATCH_SIZES)
def test_moments_four_keypoints_per_wave(pkg, patch_size):
    run(pkg, patch_size, 4)
