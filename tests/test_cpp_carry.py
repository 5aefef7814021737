"""The C++ mirror of the one-window carry entry (host/orb.hpp: orbx::localise_carried_window)
against the Python binding (orbx_carry.localise_carried_window) on the same arrays: statuses and counts, every double
as a hex float, the carried points."""
import os
import subprocess

import numpy as np
import pytest

import carry_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = R.K


@pytest.fixture(scope="module")
def mirror(pkg, tmp_path_factory):
    exe = tmp_path_factory.mktemp("carry_mirror") / "carry_mirror.bin"
    pk = os.path.join(ROOT, "visual-odometry-gpu_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(pk, "host"), "-o",
                           str(exe), os.path.join(ROOT, "tests", "cpp", "carry_mirror.cpp"), "-L" + pk, "-lorbx",
                           "-Wl,-rpath," + pk, "-Wl,-rpath,/opt/rocm/lib"])
    return str(exe)


def run(mirror, path):
    r = subprocess.run([mirror, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert lines[0][0] == "status" and lines[-2][0] == "poses" and lines[-1][0] == "points"
    records = [ln[1:] for ln in lines[1:-2]]
    assert all(ln[0] == "record" for ln in lines[1:-2])
    return (int(lines[0][1]), int(lines[0][3])), records, lines[-2][1:], [int(v) for v in lines[-1][1:]]


def blob(pts, slots, origin, tracks, seen, iterations, refine, min_inliers, seed, error, confidence):
    n_slots, n_frames = tracks.shape[:2]
    ints = b"".join(np.int32(v).tobytes() for v in (len(pts), n_slots, n_frames, iterations, refine, min_inliers))
    return (np.ascontiguousarray(K).tobytes() + ints + np.uint64(seed).tobytes() + np.float64(error).tobytes() +
            np.float64(confidence).tobytes() + np.ascontiguousarray(pts, np.float64).tobytes() +
            np.ascontiguousarray(slots, np.int32).tobytes() + np.ascontiguousarray(origin, np.int32).tobytes() +
            np.ascontiguousarray(tracks, np.float32).tobytes() + np.ascontiguousarray(seen, np.int32).tobytes())


def test_the_mirror_compiles_without_a_gpu(mirror):
    assert os.path.exists(mirror)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["clean", "few", "nothing"])
def test_localise_carried_window_mirror(pkg, mirror, tmp_path, case):
    _, old, new = R.two_generations(31, W=4, old_slots=60, fresh=8, min_seen=3)
    origin = new["origin"].copy()
    if case == "few":
        origin[3:] = -1
    args = dict(iterations=200, refine=10, min_inliers=4, seed=9, error=0.5, confidence=0.99)
    with pkg.Context(pkg.default_params("gpu")) as c:
        c.landmarks_build(K, old["tracks"][None], old["seen"][None], old["true_poses"][None])
        block = c.landmarks_fetch()
        pts, slots = block["points3"], block["slot_of_point"]
        if case == "nothing":
            pts, slots = pts[:0], slots[:0]
        want = pkg.orbx_carry.localise_carried_window(c, pts, slots, origin, new["tracks"], new["seen"], K,
                                                      prob=args["confidence"], threshold_px=args["error"],
                                                      max_iters=args["iterations"], seed=args["seed"],
                                                      refine_iters=args["refine"], min_inliers=args["min_inliers"])
    path = tmp_path / "carry.bin"
    path.write_bytes(blob(pts, slots, origin, new["tracks"], new["seen"], **args))
    (status, ok), records, poses, points = run(mirror, path)
    assert status == want["window_status"] and ok == int(status == pkg.orbx_carry.CARRY_OK)
    assert len(records) == 4
    for got, r in zip(records, want["records"]):
        assert [int(v) for v in got[:4]] == [r["status"], r["inliers"], r["iters"], r["n_corr"]]
        assert [float.fromhex(v).hex() for v in got[4:]] == [float(v).hex() for v in [r["rms_px"]] + list(r["pose6"])]
    assert [float.fromhex(v).hex() for v in poses] == [float(v).hex() for v in want["poses6"].ravel()]
    assert points == list(want["carried_point"])
    st = want["records"]["status"]
    if case == "clean":
        assert status == pkg.orbx_carry.CARRY_OK and (st == pkg.orbx_pnp.OK).all() and sum(p >= 0 for p in points) > 15
    elif case == "few":
        assert status == pkg.orbx_carry.CARRY_LOST and (st == pkg.orbx_pnp.FEW_POINTS).all()
        assert sum(p >= 0 for p in points) == 3
    else:
        assert status == pkg.orbx_carry.CARRY_LOST and (st == pkg.orbx_pnp.SKIPPED).all() and set(points) == {-1}
