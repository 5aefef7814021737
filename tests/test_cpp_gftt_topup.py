"""The C++ mirror of the masked cv::goodFeaturesToTrack and of the top-up of tracked points (host/orb.hpp: the mask
overload of orbx::goodFeaturesToTrack, orbx::top_up_keypoints), driven through
tests/cpp/gftt_topup_mirror.cpp and compared bit for bit with the numpy restatement (tests/gftt_topup_ref.py)."""
import os
import subprocess

import numpy as np
import pytest

import gftt_ref as G
import gftt_topup_ref as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    exe = tmp_path_factory.mktemp("gftt_topup_mirror") / "gftt_topup_mirror.bin"
    pk = os.path.join(ROOT, "visual-odometry-gpu_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(pk, "host"), "-o",
                           str(exe), os.path.join(ROOT, "tests", "cpp", "gftt_topup_mirror.cpp"), "-L" + pk, "-lorbx",
                           "-Wl,-rpath," + pk, "-Wl,-rpath,/opt/rocm/lib"])
    return str(exe)


@pytest.fixture(scope="module")
def crop(pkg):
    return np.ascontiguousarray(pkg.streams.load_kitti(0)[100:260, 300:620])


def run(mirror, mode, blob, tmp_path):
    path = tmp_path / (mode + ".bin")
    path.write_bytes(blob)
    r = subprocess.run([mirror, mode, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.splitlines()


def image_blob(img):
    h, w = img.shape
    return np.array([w, h], np.int32).tobytes() + img.tobytes()


def params_blob(params):
    return np.int32(params[0]).tobytes() + np.array(params[1:], np.float64).tobytes()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("params", [(2000, 0.01, 8.0), (0, 0.001, 1.0), (5, 0.01, 0.0)])
def test_good_features_to_track_with_a_mask(mirror, crop, tmp_path, params):
    """the left half plane masked out, and the strongest pixel of the right one; (0, 0.001, 1): no limit and more
    corners than the mirror's first guess of the capacity"""
    mask = np.full(crop.shape, 255, np.uint8)
    mask[:, :160] = 0
    eig = G.corner_min_eigen_val(crop)
    y, x = np.unravel_index(np.argmax(np.where(mask > 0, eig, -1)), eig.shape)
    mask[y, x] = 0
    lines = run(mirror, "mask", image_blob(crop) + mask.tobytes() + params_blob(params), tmp_path)
    got = np.array([[float.fromhex(v) for v in ln.split()] for ln in lines], np.float32).reshape(-1, 2)
    ref = T.good_features_to_track_masked(crop, mask, *params)
    assert len(ref) > 0 and ref[:, 0].min() >= 160
    assert got.shape == ref.shape and np.array_equal(bits(got), bits(ref))


@pytest.mark.parametrize("params", [(2000, 0.01, 8.0), (40, 0.01, 3.5)])
def test_top_up_keypoints(mirror, crop, tmp_path, params):
    """every third corner, moved by a sub-pixel offset, as the tracked points; one of them outside the frame"""
    rng = np.random.default_rng(5)
    c = G.good_features_to_track(crop, 2000, 0.01, 8)[::3]
    seeds = (c + rng.uniform(-0.49, 0.49, c.shape)).astype(np.float32)
    seeds[4] = (-0.25, 10.0)
    blob = image_blob(crop) + np.int32(len(seeds)).tobytes() + seeds.tobytes() + params_blob(params)
    lines = run(mirror, "topup", blob, tmp_path)
    carried = int(lines[0])
    rows = [ln.split() for ln in lines[1:]]
    pts = np.array([[float.fromhex(r[0]), float.fromhex(r[1])] for r in rows], np.float32).reshape(-1, 2)
    origin = np.array([int(r[2]) for r in rows], np.int32)
    want_pts, want_origin, want_carried = T.top_up(crop, seeds, *params)
    assert want_carried == min(len(seeds) - 1, params[0]) and 4 not in want_origin
    if params[0] == 2000:
        assert len(want_pts) > want_carried
    assert carried == want_carried and np.array_equal(origin, want_origin)
    assert pts.shape == want_pts.shape and np.array_equal(bits(pts), bits(want_pts))
