"""The C++ mirror of the views build (host/orb.hpp: orbx::LandmarkOptions and the overload of
orbx::run_bundle_adjustment_on_tracks taking it) against the Python binding's route
(orbx_lm.bundle_adjust_tracks_views) on the same blocks: status, summary, refined landmarks and their slots bit for
bit (hex doubles).  Default options are the overload without them."""
import os
import subprocess

import numpy as np
import pytest

import landmarks_ref as R
from test_cpp_landmarks import cam_to_world, hexes, scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = R.K_KITTI


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    exe = tmp_path_factory.mktemp("lm_views_mirror") / "lm_views_mirror.bin"
    pk = os.path.join(ROOT, "visual-odometry-gpu_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(pk, "host"), "-o",
                           str(exe), os.path.join(ROOT, "tests", "cpp", "lm_views_mirror.cpp"), "-L" + pk, "-lorbx",
                           "-Wl,-rpath," + pk, "-Wl,-rpath,/opt/rocm/lib"])
    return str(exe)


@pytest.mark.parametrize("mode,gate", [(2, 3.0), (1, 0.0), (0, 0.0)])
def test_run_bundle_adjustment_on_tracks_with_options(pkg, mirror, tmp_path, mode, gate):
    sc = scene("near")
    W, n = 5, len(sc["seen"])
    start = np.array([cam_to_world(q) for q in sc["poses"]])
    blob = K.tobytes() + np.int32(W).tobytes() + start.tobytes() + np.int32(n).tobytes()
    blob += sc["tracks"].tobytes() + sc["seen"].tobytes()
    path = tmp_path / "near.bin"
    path.write_bytes(blob)
    r = subprocess.run([mirror, str(path), str(mode), repr(gate)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    blocks = np.array([hexes(ln[2:]) for ln in lines if ln[0] == "block"])
    head = next(ln for ln in lines if ln[0] == "ran")
    info = {head[i]: head[i + 1] for i in range(0, len(head), 2)}
    pts = np.array([hexes(ln[2:]) for ln in lines if ln[0] == "point"]).reshape(-1, 3)
    slots = np.array([int(ln[1]) for ln in lines if ln[0] == "point"])
    with pkg.Context(pkg.default_params("gpu")) as c:
        _, want_s, st, want_x, want_slot = pkg.orbx_lm.bundle_adjust_tracks_views(c, K, sc["tracks"], sc["seen"],
                                                                                 blocks, mode, gate)
        if (mode, gate) == (0, 0.0):
            _, plain_s, plain_st, plain_x, plain_slot = c.bundle_adjust_tracks(K, sc["tracks"], sc["seen"], blocks)
            assert (plain_s, plain_st) == (want_s, st) and np.array_equal(plain_slot, want_slot)
            assert np.array_equal(plain_x.view(np.uint64), want_x.view(np.uint64))
    assert info["ran"] == "1" and int(info["status"]) == st == R.OK and int(info["landmarks"]) == len(want_x) > 200
    assert (int(info["termination"]), int(info["iterations"]), int(info["steps"])) == (
        want_s["termination"], want_s["iterations"], want_s["successful_steps"])
    assert float.fromhex(info["initial"]).hex() == want_s["initial_cost"].hex()
    assert float.fromhex(info["final"]).hex() == want_s["final_cost"].hex()
    assert np.array_equal(slots, want_slot) and np.array_equal(pts.view(np.uint64), want_x.view(np.uint64))
