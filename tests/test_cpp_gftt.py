"""The C++ mirror of cv::goodFeaturesToTrack and of run_bundle_adjustment's initial-keypoint branch
(host/orb.hpp: orbx::goodFeaturesToTrack, orbx::initial_keypoints; src/with_bundle_adjustment.cpp:586-593), driven
through tests/cpp/gftt_mirror.cpp and compared bit for bit with the numpy restatement (tests/gftt_ref.py)."""
import os
import subprocess

import numpy as np
import pytest

import gftt_ref as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    exe = tmp_path_factory.mktemp("gftt_mirror") / "gftt_mirror.bin"
    pk = os.path.join(ROOT, "visual-odometry-gpu_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(pk, "host"), "-o",
                           str(exe), os.path.join(ROOT, "tests", "cpp", "gftt_mirror.cpp"), "-L" + pk, "-lorbx",
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
    pts = [[float.fromhex(v) for v in ln.split()] for ln in r.stdout.splitlines()]
    return np.array(pts, np.float32).reshape(-1, 2)


def image_blob(img):
    h, w = img.shape
    return np.array([w, h], np.int32).tobytes() + img.tobytes()


@pytest.mark.parametrize("params", [(2000, 0.01, 8.0), (0, 0.001, 1.0), (5, 0.01, 0.0)])
def test_good_features_to_track(mirror, crop, tmp_path, params):
    """(0, 0.001, 1): no limit and more corners than the mirror's first guess of the capacity."""
    blob = image_blob(crop) + np.int32(params[0]).tobytes() + np.array(params[1:], np.float64).tobytes()
    got = run(mirror, "gftt", blob, tmp_path)
    ref = G.good_features_to_track(crop, *params)
    assert len(ref) > 0 and got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_initial_keypoints_from_observations(mirror, crop, tmp_path):
    """observations of frame 0 present: they are the keypoints, as (float)x, (float)y; nothing is detected"""
    obs = np.array([[10.25, 20.5], [300.123456789, 7.0], [0.1, 159.9]], np.float64)
    got = run(mirror, "init", image_blob(crop) + np.int32(len(obs)).tobytes() + obs.tobytes(), tmp_path)
    assert np.array_equal(got.view(np.uint32), obs.astype(np.float32).view(np.uint32))


def test_initial_keypoints_detected(mirror, crop, tmp_path):
    """no observations: goodFeaturesToTrack(img0, 2000, 0.01, 8)"""
    got = run(mirror, "init", image_blob(crop) + np.int32(0).tobytes(), tmp_path)
    ref = G.good_features_to_track(crop, 2000, 0.01, 8)
    assert len(ref) > 100 and got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32))
