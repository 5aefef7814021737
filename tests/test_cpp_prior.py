"""The C++ mirror of the solve with landmark priors (host/orb.hpp: orbx::bundle_adjust_with_priors; DESIGN.md §9
rank 20) against the Python binding (orbx_prior.bundle_adjust_prior) on the same arrays: the summary and every double
as a hex float."""
import os
import subprocess

import numpy as np
import pytest

import test_ba as B
from test_ba_prior import START_ANCHOR, START_GIVEN, mixed_priors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = B.K_KITTI


@pytest.fixture(scope="module")
def mirror(pkg, tmp_path_factory):
    exe = tmp_path_factory.mktemp("prior_mirror") / "prior_mirror.bin"
    pk = os.path.join(ROOT, "visual-odometry-gpu_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(pk, "host"), "-o",
                           str(exe), os.path.join(ROOT, "tests", "cpp", "prior_mirror.cpp"), "-L" + pk, "-lorbx",
                           "-Wl,-rpath," + pk, "-Wl,-rpath,/opt/rocm/lib"])
    return str(exe)


def blob(win, anchors, weights, start, max_iters, delta):
    n_priors = 0 if anchors is None else len(anchors)
    ints = np.array([len(win["poses0"]), len(win["pts0"]), len(win["obs_point"]), n_priors, start, max_iters], np.int32)
    out = np.ascontiguousarray(K).tobytes() + ints.tobytes() + np.float64(delta).tobytes()
    for a, dt in ((win["poses0"], np.float64), (win["pts0"], np.float64), (win["obs_point"], np.int32),
                  (win["obs_pose"], np.int32), (win["obs_xy"], np.float64)):
        out += np.ascontiguousarray(a, dt).tobytes()
    if n_priors:
        out += np.ascontiguousarray(anchors, np.float64).tobytes() + np.ascontiguousarray(weights, np.float64).tobytes()
    return out


def test_the_mirror_compiles_without_a_gpu(mirror):
    assert os.path.exists(mirror)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["mixed", "anchor start", "no priors", "iteration limit"])
def test_bundle_adjust_with_priors_mirror(pkg, mirror, tmp_path, case):
    win = B.make_window(1500, 5, 120, sigma=0.3, outliers=0.05)
    anchors, weights = mixed_priors(win, 1501)
    start, max_iters = (START_ANCHOR if case in ("anchor start", "iteration limit") else START_GIVEN), 200
    if case == "no priors":
        anchors = weights = None
    if case == "iteration limit":
        max_iters = 1
    with pkg.Context(pkg.default_params("gpu")) as c:
        poses, pts, s = pkg.orbx_prior.bundle_adjust_prior(c, K, win["poses0"], win["pts0"], win["obs_point"],
                                                           win["obs_pose"], win["obs_xy"], anchors, weights, start,
                                                           huber_delta=1.5, max_iters=max_iters)
    path = tmp_path / "prior.bin"
    path.write_bytes(blob(win, anchors, weights, start, max_iters, 1.5))
    r = subprocess.run([mirror, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert [ln[0] for ln in lines] == ["summary", "poses", "points"]
    assert [int(v) for v in lines[0][1:4]] == [s["termination"], s["iterations"], s["successful_steps"]]
    assert [float.fromhex(v).hex() for v in lines[0][4:6]] == [float(s["initial_cost"]).hex(), float(s["final_cost"]).hex()]
    assert int(lines[0][7]) == int(s["termination"] == B.CONVERGENCE)
    assert [float.fromhex(v).hex() for v in lines[1][1:]] == [float(v).hex() for v in poses.ravel()]
    assert [float.fromhex(v).hex() for v in lines[2][1:]] == [float(v).hex() for v in pts.ravel()]
    if case == "iteration limit":  # rule P5: the given blocks come back, not the anchors
        assert s["termination"] == B.NO_CONVERGENCE and np.array_equal(pts, win["pts0"])
    else:
        assert s["termination"] == B.CONVERGENCE
