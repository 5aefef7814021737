"""The sequential restatement of the projection (tests/cpp/search_sequential.cpp on csrc/orbx_search_math.h; DESIGN.md
§9 rank 21 rules P1-P5) against the numpy restatement tests/search_ref.py on the scene of the device test, without a
GPU; the figure measured here sets the tolerance of the device-against-numpy comparison (search_seq.TOLERANCE_PX).
Further down the C++ mirror of the two host entries (host/orb.hpp: orbx::project_landmarks, orbx::reassociate_gated)
against the Python binding on the same arrays."""
import os
import subprocess

import numpy as np
import pytest

import carry_ref as CR
import landmarks_seq as LS
import search_ref as S
import search_seq as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = CR.K
W, H, MARGIN, CAP = S.IMG_W, S.IMG_H, S.PROJ_MARGIN, S.PROJ_CAP


@pytest.fixture(scope="module")
def seq(tmp_path_factory):
    return Q.compile_so(tmp_path_factory.mktemp("search_seq"))


@pytest.fixture(scope="module")
def lm(tmp_path_factory):
    return LS.compile_so(tmp_path_factory.mktemp("lm_seq_search"), "lm_sequential")


@pytest.fixture(scope="module")
def scene(lm):
    sc = S.projection_scene()
    poses, tracks, seen = CR.stack_old(sc["olds"])
    sc["block"] = LS.seq_build(lm, K, poses, tracks, seen)
    return sc


def test_the_scene_stays_clear_of_every_state_boundary(scene):
    """the numpy reference alone puts no slot within 1e-6 of depth 0 or of a margin line: no slot is left out when
    states are compared exactly"""
    detail = []
    ref = S.project(scene["block"], scene["poses6"], K, W, H, MARGIN, CAP, detail=detail)
    S.check_projection_scene(scene["block"], ref)
    assert sum(len(d) for d in detail) >= 60
    assert S.boundary_distance(detail, W, H, MARGIN) > 1e-6


def test_sequential_against_numpy(seq, scene):
    ref = S.project(scene["block"], scene["poses6"], K, W, H, MARGIN, CAP)
    got = Q.project(seq, scene["block"], scene["poses6"], K, W, H, MARGIN, CAP)
    assert got["state"].tolist() == ref["state"].tolist() and got["count"].tolist() == ref["count"].tolist()
    ok = ref["state"] == S.PROJ_OK
    assert not got["xy"][~ok].any() and not got["depth"][~ok].any()
    worst = max(float(np.abs(got["xy"] - ref["xy"]).max()), float(np.abs(got["depth"] - ref["depth"]).max()))
    print("largest difference between the sequential program and numpy: %.3g" % worst)
    # the figure in search_seq.py is this one, rounded up; numpy's sin and cos may differ in the last place from one
    # processor to the next, which moves a pixel by another unit in the last place
    assert worst <= 2 * Q.MEASURED_PX
    # a pose stride above 6 reads the same poses
    wide = np.full((5, 4, 6), 7.0)
    wide[:, 3] = scene["poses6"]
    again = Q.project(seq, scene["block"], wide.reshape(-1)[18:], K, W, H, MARGIN, CAP, pose_stride=24)
    assert all(again[k].tobytes() == got[k].tobytes() for k in got)


def test_the_gate_of_the_sequential_program_is_rule_l(seq):
    out = float(np.nextafter(13.0, np.inf))
    assert Q.in_gate(seq, 10.0, 20.0, 13.0, 24.0, 5.0) and not Q.in_gate(seq, 10.0, 20.0, out, 24.0, 5.0)
    rng = np.random.default_rng(3)
    q = rng.uniform(0, 100, (500, 2)).astype(np.float32)
    t = q + rng.normal(0, 4.0, (500, 2))
    for i in range(500):
        assert Q.in_gate(seq, q[i, 0], q[i, 1], t[i, 0], t[i, 1], 5.5) == bool(S.gate_candidates(q[i], t[i], 5.5)[0])


# ---- the C++ mirror ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mirror(pkg, tmp_path_factory):
    exe = tmp_path_factory.mktemp("search_mirror") / "search_mirror.bin"
    pk = os.path.join(ROOT, "visual-odometry-gpu_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(pk, "host"), "-o",
                           str(exe), os.path.join(ROOT, "tests", "cpp", "search_mirror.cpp"), "-L" + pk, "-lorbx",
                           "-Wl,-rpath," + pk, "-Wl,-rpath,/opt/rocm/lib"])
    return str(exe)


def test_the_mirror_compiles_without_a_gpu(mirror):
    assert os.path.exists(mirror)


@pytest.mark.gpu
def test_the_mirror_equals_the_binding(pkg, mirror, scene, tmp_path):
    block = scene["block"]
    p0, p1 = int(block["point_offset"][0]), int(block["point_offset"][1])
    pts, slot = block["points3"][p0:p1], block["slot_of_point"][p0:p1]
    g = S.gated_windows(70, 300, (96, 64), 41)
    params = dict(radius_px=8.0, ratio=0.8, max_distance=64, accept_lone=1, unique=1)
    with pkg.Context(pkg.default_params("gpu")) as c:
        proj = pkg.orbx_search.project_landmarks_host(c, pts, slot, CAP, K, scene["poses6"][0], W, H, MARGIN)
        gated = pkg.orbx_search.reassociate_gated_host(c, g["qdesc"][0], g["qstate"][0], g["qxy"][0], g["tdesc"][0],
                                                       g["tstate"][0], g["txy"][0], g["tpstate"][0], **params)
    ints = np.array([len(pts), CAP, W, H, 70, 300, params["max_distance"], params["accept_lone"], params["unique"]],
                    np.int32)
    dbl = np.array([MARGIN, params["radius_px"], params["ratio"]], np.float64)
    blob = ints.tobytes() + dbl.tobytes() + np.ascontiguousarray(K, np.float64).tobytes()
    for a, dt in ((scene["poses6"][0], np.float64), (pts, np.float64), (slot, np.int32), (g["qdesc"][0], np.uint8),
                  (g["qstate"][0], np.int32), (g["qxy"][0], np.float32), (g["tdesc"][0], np.uint8),
                  (g["tstate"][0], np.int32), (g["txy"][0], np.float64), (g["tpstate"][0], np.int32)):
        blob += np.ascontiguousarray(a, dt).tobytes()
    path = tmp_path / "search.bin"
    path.write_bytes(blob)
    r = subprocess.run([mirror, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines()}
    assert sorted(lines) == ["candidates", "count", "depth", "dist", "origin", "pcount", "state", "xy"]
    assert [float.fromhex(v).hex() for v in lines["xy"]] == Q.hexes(proj["xy"])
    assert [float.fromhex(v).hex() for v in lines["depth"]] == Q.hexes(proj["depth"])
    assert [int(v) for v in lines["state"]] == proj["state"].tolist() and int(lines["pcount"][0]) == proj["count"] > 0
    for k in ("origin", "dist", "candidates"):
        assert [int(v) for v in lines[k]] == gated[k].tolist(), k
    assert int(lines["count"][0]) == gated["count"] > 5
