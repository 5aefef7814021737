"""Edge cases of the per-level selection (k_level_select) and of the batched describe kernel (k_describe2),
through the C ABI against the oracle, bit for bit: keypoints on every level's border (the one-pixel
REFLECT_101 Harris windows and the non-interior describe path), keypoint counts that leave partial
workgroups, every Harris window, both select modes, saturated content with tied Harris responses, the
host-record path and the single-frame call.
"""
import importlib.util
import os

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "fuzz_parity", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz_parity.py"))
F = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(F)


def edge_image(seed, h, w, saturated=False):
    """Noise with strong structure in the outer 20 px of the frame, so that every level has keypoints at its border."""
    rng = np.random.default_rng(seed)
    img = 100.0 + 20.0 * rng.standard_normal((h, w))
    band = np.zeros((h, w), bool)
    band[:20], band[-20:], band[:, :20], band[:, -20:] = True, True, True, True
    img[band] = rng.integers(0, 256, int(band.sum()))
    if saturated:  # the kind of tools/fuzz_parity.py that makes many Harris responses tie
        img = np.where(img > 128, 255, 0) + rng.integers(0, 2, (h, w))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def reference(img, kw, mode):
    return O.detect_and_compute_gpu(img, O.gpu_params(**kw)) if mode == 0 else F.rowmajor_ref(img, kw)


def run_batch(pkg, imgs, kw, mode, host=False):
    B, h, w = imgs.shape
    p = pkg.default_params("gpu", max_width=w, max_height=h, max_batch=B, select_mode=mode, **kw)
    with pkg.Context(p) as c:
        cap = max(c.plan(w, h)["out_capacity"], 1)
        c.set_host_results(host)
        c.batch_host(imgs)
        hv = F.host_record(c) if host else None
        r = c.batch_fetch(0, B, cap)
        single = c.detect_and_compute(imgs[0])
    for i in range(B):
        ref = reference(imgs[i], kw, mode)
        n = int(r["counts"][i])
        got = dict(count=n, kps=r["kps"][i, :n], kps_level=r["kps_level"][i, :n], levels=r["levels"][i, :n],
                   angles=r["angles"][i, :n], responses=r["responses"][i, :n], desc=r["desc"][i, :n])
        F.check(got, ref, (i, kw, mode))
        if i == 0:
            F.check(single, ref, ("single", kw, mode))
        if hv is not None:
            assert int(hv["counts"][i]) == n
            assert np.array_equal(hv["kps16"][i, :n].astype(np.int32), r["kps"][i, :n])
            assert np.array_equal(hv["angles"][i, :n].view(np.uint32), r["angles"][i, :n].view(np.uint32))
            assert np.array_equal(hv["desc"][i, :n], r["desc"][i, :n])
    return r


BASE = dict(nfeatures=500, nlevels=4, scale_factor=1.2, threshold=20, n=9, nms_window=3, patch_size=31,
            harris_window=7, harris_k=0.04, blur_levels=0, blur_kind=0)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("harris_window", [3, 5, 7])
@pytest.mark.parametrize("patch_size", [1, 9, 31, 41])
def test_border_keypoints(pkg, mode, harris_window, patch_size):
    imgs = np.stack([edge_image(10 * patch_size + harris_window + k, 150, 230) for k in range(3)])
    kw = dict(BASE, harris_window=harris_window, patch_size=patch_size)
    r = run_batch(pkg, imgs, kw, mode)
    assert int(r["counts"].min()) > 16


@pytest.mark.parametrize("nfeatures", [1, 2, 3, 4, 5, 17, 37])
def test_partial_workgroups(pkg, nfeatures):
    imgs = np.stack([edge_image(nfeatures + k, 120, 180) for k in range(2)])
    kw = dict(BASE, nfeatures=nfeatures, nlevels=1 if nfeatures <= 5 else 3)
    r = run_batch(pkg, imgs, kw, 0)
    assert int(r["counts"].max()) > 0


@pytest.mark.parametrize("harris_window", [3, 5, 7])
def test_tied_harris_responses(pkg, harris_window):
    imgs = np.stack([edge_image(77 + k, 200, 260, saturated=True) for k in range(3)])
    kw = dict(BASE, nfeatures=2000, nlevels=5, harris_window=harris_window, threshold=12)
    run_batch(pkg, imgs, kw, 0)


def test_host_results_batch(pkg):
    imgs = np.stack([edge_image(300 + k, 376, 600) for k in range(5)])
    kw = dict(BASE, nfeatures=1000, nlevels=8, blur_levels=2)
    run_batch(pkg, imgs, kw, 0, host=True)
