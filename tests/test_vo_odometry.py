"""examples/vo_odometry.cpp: the reference's matching VO loop (VisualOdom::run, feature_matching.cpp:43-107) end to
end on liborbx -- PNG frames, calib.txt and a poses file of a KITTI sequence directory -> ORB -> 2-NN + ratio test ->
get_pose -> get_scale -> pose chaining -> the three files savePaths writes."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from test_kitti_io import write_png

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "visual-odometry-gpu_amd")


@pytest.fixture(scope="module")
def example(tmp_path_factory):
    """The example, compiled here against the built liborbx.so (the way tests/test_pose.py compiles its mirror)."""
    exe = tmp_path_factory.mktemp("vo_odometry") / "vo_odometry.bin"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", str(exe),
                           os.path.join(ROOT, "examples", "vo_odometry.cpp"), "-L" + PKG, "-lorbx", "-lz",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return str(exe)


def test_example_builds(pkg, example):
    assert os.path.exists(example)
    r = subprocess.run([example], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


@pytest.mark.gpu
def test_matching_loop_on_the_golden_frames(pkg, example, tmp_path):
    n = 6
    seq = tmp_path / "data_odometry_gray" / "dataset" / "sequences" / "00"
    (seq / "image_0").mkdir(parents=True)
    for i in range(n):  # the two golden frames alternating: the camera steps forth and back
        write_png(seq / "image_0" / ("%06d.png" % i), O.load_kitti(i % 2), 0, (0, 1, 2), idat_split=2)
    P = np.array([[718.856, 0, 607.1928, 0], [0, 718.856, 185.2157, 0], [0, 0, 1, 0]])
    (seq / "calib.txt").write_text("P0: " + " ".join("%.12e" % v for v in P.ravel()) + "\n")
    poses_dir = tmp_path / "data_odometry_poses" / "dataset" / "poses"
    poses_dir.mkdir(parents=True)
    gt = np.tile(np.eye(4)[:3], (n, 1, 1))
    gt[:, 0, 3] = 2.0
    gt[1::2, 2, 3] = 0.86  # odd frames: 0.86 units ahead
    (poses_dir / "00.txt").write_text("\n".join(" ".join("%.9e" % v for v in T.ravel()) for T in gt) + "\n")
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([example, str(tmp_path), "00", "100", "3000", str(out)], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines() if ln and ln[0].isdigit()]
    assert len(rows) == n and int(rows[0][1]) > 2000
    assert all(int(row[1]) > 500 for row in rows[1:])  # matches per pair
    # savePaths: one row per frame in the paths, one per pair in scale.txt
    gt_path, est_path, scale = (np.loadtxt(out / f, ndmin=2) for f in ("gt_path.txt", "est_path.txt", "scale.txt"))
    assert gt_path.shape == (n, 2) and est_path.shape == (n, 2) and scale.shape == (n - 1, 2)
    assert np.allclose(gt_path, gt[:, [0, 2], 3], rtol=1e-5)
    assert np.array_equal(est_path[0], gt_path[0])  # cur_pose = gt_pose at frame 0
    assert np.allclose(scale[:, 0], 0.86, rtol=1e-5)
    assert scale[0, 1] == 1.0  # no previous points at the first pair
    assert ((scale[:, 1] >= 0.1) & (scale[:, 1] <= 5.0)).all()
    assert np.isfinite(est_path).all()
    # each estimated step has the length of its scale (|t| = 1), up to the files' 6 significant digits in x and z
    step = np.linalg.norm(np.diff(est_path, axis=0), axis=1)
    assert (step <= scale[:, 1] * (1 + 1e-4) + 1e-4).all()
    # the files re-read through kitti_io.hpp (the driver of tests/test_kitti_io.py parses and re-saves them)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "test_kitti_io.bin"],
                          stdout=subprocess.DEVNULL)
    names = ("gt_path.txt", "est_path.txt", "scale.txt")
    again = [tmp_path / ("again_" + f) for f in names]
    subprocess.check_call([os.path.join(ROOT, "tests", "cpp", "test_kitti_io.bin"), "paths"] +
                          [str(out / f) for f in names] + [str(a) for a in again])
    for f, a in zip(names, again):
        assert (out / f).read_bytes() == a.read_bytes(), f
