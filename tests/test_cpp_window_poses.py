"""The C++ mirror of the window-odometry route (host/orb.hpp: orbx::run_window_odometry_on_tracks; DESIGN.md §9 rank
14) against the Python route (orbx_vo.window_odometry_tracks) on one synthetic window: statuses, summary, the gated
poses and the updated flags bit for bit (hex doubles)."""
import os
import subprocess

import numpy as np
import pytest

import landmarks_ref as R
import window_poses_ref as WR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = R.K_KITTI


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    exe = tmp_path_factory.mktemp("wp_mirror") / "wp_mirror.bin"
    pk = os.path.join(ROOT, "visual-odometry-gpu_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(pk, "host"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "wp_mirror.cpp"), "-L" + pk, "-lorbx",
                           "-Wl,-rpath," + pk, "-Wl,-rpath,/opt/rocm/lib"])
    return str(exe)


def test_run_window_odometry_on_tracks(pkg, mirror, tmp_path):
    sc = R.make_scene(700, W=5, slots=300, sigma=0.1, min_seen=2)
    W, n = 5, len(sc["seen"])
    pose0 = WR.rigid(WR.rot([0.2, 1.0, -0.1], 0.3), [1.0, -2.0, 0.5])
    scale0 = 0.8
    blob = K.tobytes() + pose0.tobytes() + np.float64(scale0).tobytes() + np.int32(W).tobytes() + np.int32(n).tobytes()
    blob += sc["tracks"].tobytes() + sc["seen"].tobytes()
    path = tmp_path / "window.bin"
    path.write_bytes(blob)
    r = subprocess.run([mirror, "window", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    head = next(ln for ln in lines if ln[0] == "ran")
    info = {head[i]: head[i + 1] for i in range(1, len(head), 2)}
    poses = np.array([[float.fromhex(v) for v in ln[4:]] for ln in lines if ln[0] == "pose"]).reshape(W, 4, 4)
    updated = np.array([int(ln[3]) for ln in lines if ln[0] == "pose"], np.uint8)
    with pkg.Context(pkg.default_params("gpu")) as c:
        want = pkg.orbx_vo.window_odometry_tracks(c, K, sc["tracks"], sc["seen"], pose0, scale0)
    s = want["summary"]
    assert (int(info["wp_status"]), int(info["lm_status"])) == (want["wp_status"], want["lm_status"]) == (0, R.OK)
    assert (int(info["termination"]), int(info["iterations"]), int(info["steps"])) == (
        s["termination"], s["iterations"], s["successful_steps"])
    assert s["termination"] == pkg.orbx.BA_CONVERGENCE and s["iterations"] >= 1
    assert float.fromhex(info["initial"]).hex() == s["initial_cost"].hex()
    assert float.fromhex(info["final"]).hex() == s["final_cost"].hex()
    assert np.array_equal(updated, want["updated"]) and updated.all()
    assert poses.tobytes() == want["poses4x4"].tobytes()
    # the window starts at pose0 (through its block and back) and moves on from there
    assert np.allclose(poses[0], pose0, rtol=0, atol=1e-12)
    assert np.linalg.norm(poses[1][:3, 3] - poses[0][:3, 3]) > 0.1 * scale0
