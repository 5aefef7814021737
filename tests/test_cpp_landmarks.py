"""The C++ mirror of the device landmark route (host/orb.hpp: orbx::run_bundle_adjustment_on_tracks; DESIGN.md §9
rank 10) against the Python binding's route (Context.bundle_adjust_tracks) on the same blocks: summary, refined
landmarks and their slots bit for bit (hex doubles), the write-back gate restated in numpy."""
import os
import subprocess

import numpy as np
import pytest

import landmarks_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = R.K_KITTI


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    exe = tmp_path_factory.mktemp("lm_mirror") / "lm_mirror.bin"
    pk = os.path.join(ROOT, "visual-odometry-gpu_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(pk, "host"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "lm_mirror.cpp"), "-L" + pk, "-lorbx",
                           "-Wl,-rpath," + pk, "-Wl,-rpath,/opt/rocm/lib"])
    return str(exe)


def cam_to_world(pose6):
    Rm = R.rodrigues(pose6[:3])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rm.T, -Rm.T @ pose6[3:]
    return T


def scene(name):
    """`near`: every pose passes the gate.  `scaled`: the same window in units 60 times as large (steps of 30-90,
    inside the baseline gate of 100; the pixels do not change) whose pose 3 starts 60 units off: the solve moves it
    back by more than 50, so the gate rejects it."""
    sc = R.make_scene(700, W=5, slots=300, sigma=0.1, min_seen=2, pose_pert=0.003)
    if name == "scaled":
        sc = dict(sc, poses=sc["poses"].copy())
        sc["poses"][:, 3:] *= 60.0
        sc["poses"][3, 3:] += 60.0 * np.array([0.6, 0.0, 0.8])
    return sc


def hexes(words):
    return np.array([float.fromhex(v) for v in words])


@pytest.mark.parametrize("name", ["near", "scaled"])
def test_run_bundle_adjustment_on_tracks(pkg, mirror, tmp_path, name):
    sc = scene(name)
    W, n = 5, len(sc["seen"])
    start = np.array([cam_to_world(q) for q in sc["poses"]])
    blob = K.tobytes() + np.int32(W).tobytes() + start.tobytes() + np.int32(n).tobytes()
    blob += sc["tracks"].tobytes() + sc["seen"].tobytes()
    path = tmp_path / (name + ".bin")
    path.write_bytes(blob)
    r = subprocess.run([mirror, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    blocks = np.array([hexes(ln[2:]) for ln in lines if ln[0] == "block"])
    head = next(ln for ln in lines if ln[0] == "ran")
    info = {head[i]: head[i + 1] for i in range(0, len(head), 2)}
    poses = np.array([hexes(ln[4:]) for ln in lines if ln[0] == "pose"]).reshape(W, 4, 4)
    updated = np.array([int(ln[3]) for ln in lines if ln[0] == "pose"])
    pts = np.array([hexes(ln[2:]) for ln in lines if ln[0] == "point"]).reshape(-1, 3)
    slots = np.array([int(ln[1]) for ln in lines if ln[0] == "point"])
    # the blocks the mirror made of the 4 x 4 poses are the scene's, up to the round trip through the matrix
    assert np.allclose(blocks, sc["poses"], rtol=0, atol=1e-9 * max(1.0, np.abs(sc["poses"]).max()))
    # the Python binding's route on those blocks: equal bits
    with pkg.Context(pkg.default_params("gpu")) as c:
        want_p, want_s, st, want_x, want_slot = c.bundle_adjust_tracks(K, sc["tracks"], sc["seen"], blocks)
    assert info["ran"] == "1" and int(info["status"]) == st == R.OK and int(info["landmarks"]) == len(want_x) > 200
    assert (int(info["termination"]), int(info["iterations"]), int(info["steps"])) == (
        want_s["termination"], want_s["iterations"], want_s["successful_steps"])
    assert int(info["termination"]) == pkg.orbx.BA_CONVERGENCE
    assert float.fromhex(info["initial"]).hex() == want_s["initial_cost"].hex()
    assert float.fromhex(info["final"]).hex() == want_s["final_cost"].hex()
    assert want_s["final_cost"] < want_s["initial_cost"]
    assert np.array_equal(slots, want_slot) and np.array_equal(pts.view(np.uint64), want_x.view(np.uint64))
    # the write-back gate (angle < 0.5 rad, |dt| < 50), restated in numpy on the binding's blocks
    flags, want = [], []
    for i in range(W):
        angle = np.linalg.norm(R.rotvec(R.rodrigues(want_p[i, :3]) @ R.rodrigues(blocks[i, :3]).T))
        ok = angle < 0.5 and np.linalg.norm(want_p[i, 3:] - blocks[i, 3:]) < 50.0
        flags.append(int(ok))
        want.append(cam_to_world(want_p[i]) if ok else start[i])
    assert np.array_equal(updated, flags)
    assert np.allclose(poses, np.array(want), rtol=0, atol=1e-9 * max(1.0, np.abs(start).max()))
    if name == "near":
        assert np.all(updated == 1)
    else:
        assert list(updated) == [1, 1, 1, 0, 1], updated
        assert np.array_equal(poses[3].view(np.uint64), start[3].view(np.uint64))
