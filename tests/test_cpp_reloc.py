"""The C++ mirror of rank 19 (host/orb.hpp: orbx::Feature2D::compute, orbx::describe_points, orbx::reassociate; DESIGN.md
§9 rank 19): the layout pins of the two views of include/orbx_reloc.h without a GPU, and on the GPU compute() on the
320 x 160 crop removing exactly the keypoints that are not ORBX_PD_OK and returning rows byte-equal to
orbx_describe_points through the Python binding."""
import os
import subprocess

import numpy as np
import pytest

import reassoc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mirror(pkg, tmp_path_factory):
    exe = tmp_path_factory.mktemp("reloc_mirror") / "reloc_mirror.bin"
    pk = os.path.join(ROOT, "visual-odometry-gpu_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(pk, "host"), "-o",
                           str(exe), os.path.join(ROOT, "tests", "cpp", "reloc_mirror.cpp"), "-L" + pk, "-lorbx",
                           "-Wl,-rpath," + pk, "-Wl,-rpath,/opt/rocm/lib"])
    return str(exe)


def test_the_layout_pins_of_the_two_views(pkg, mirror):
    """the static_asserts compiled; the printed numbers are the ctypes structures' too"""
    import ctypes as C

    r = subprocess.run([mirror, "pins"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = dict((ln.split()[0], [int(v) for v in ln.split()[1:]]) for ln in r.stdout.splitlines())
    o = pkg.orbx_reloc
    pv, rv = o.PointDescriptorsView, o.ReassociateView
    assert lines["orbx_point_descriptors_view"] == [C.sizeof(pv), pv.slot_capacity.offset, pv.n.offset] == [40, 32, 36]
    assert lines["orbx_reassociate_view"] == [C.sizeof(rv), rv.q_capacity.offset, rv.t_capacity.offset,
                                              rv.n_windows.offset] == [40, 24, 28, 32]


@pytest.mark.gpu
def test_compute_removes_what_cannot_be_described(pkg, oracle, mirror, tmp_path):
    crop = oracle.load_kitti(0)[100:260, 300:620].copy()
    h, w = crop.shape
    rng = np.random.default_rng(23)
    pts = np.float32([[20.5, 20.0], [21.5, 20.0], [19.0, 80.0], [299.0, 139.0], [300.0, 139.0], [np.nan, 4.0],
                      [-3.0, 50.0], [400.0, 50.0], [150.25, 70.75]])
    pts = np.concatenate([pts, np.c_[rng.uniform(0, w - 1, 40), rng.uniform(0, h - 1, 40)].astype(np.float32)])
    path = tmp_path / "reloc.bin"
    path.write_bytes(np.int32([w, h, len(pts)]).tobytes() + crop.tobytes() + pts.tobytes())
    r = subprocess.run([mirror, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    with pkg.Context(pkg.default_params("gpu", max_width=w, max_height=h)) as ctx:
        want = pkg.orbx_reloc.describe_points_host(ctx, crop, pts)
        ok = np.flatnonzero(want["state"] == R.PD_OK)
        self_match = pkg.orbx_reloc.reassociate_host(ctx, want["desc"], want["state"], want["desc"], want["state"])
    assert want["state"][:9].tolist() == [2, 2, 1, 2, 1, 0, 0, 0, 2] and 20 < len(ok) < len(pts)
    comp = [ln for ln in lines if ln[0] == "compute"]
    assert [int(ln[1]) for ln in comp] == ok.tolist()  # exactly the OK keypoints, in their order
    for ln, i in zip(comp, ok):
        deg = np.float32(want["angle"][i]) * np.float32(57.29577951308232)
        deg = deg + np.float32(360) if deg < 0 else deg
        deg = deg - np.float32(360) if deg >= np.float32(360) else deg
        assert float.fromhex(ln[2]) == float(deg) and 0.0 <= float(deg) < 360.0
        assert int(ln[3]) == i % 3  # the octave is left as it was
        assert bytes.fromhex(ln[4]) == want["desc"][i].tobytes()
    desc = [ln for ln in lines if ln[0] == "describe"]
    assert len(desc) == len(pts)
    for i, ln in enumerate(desc):
        assert int(ln[1]) == want["state"][i]
        assert np.float32(float.fromhex(ln[2])).tobytes() == want["angle"][i].tobytes()
        assert bytes.fromhex(ln[3]) == want["desc"][i].tobytes()
    origin = [ln for ln in lines if ln[0] == "origin"][0]
    assert int(origin[1]) == self_match["count"] and [int(v) for v in origin[2:]] == self_match["origin"].tolist()
    assert self_match["count"] > 20 and all(self_match["origin"][q] in (q, -1) for q in range(len(pts)))
