"""The C++ mirror of trackPointsAcrossWindow with the forward-backward check (host/orb.hpp),
driven through tests/cpp/lk_fb_mirror.cpp: the one-launch function returns exactly what the pair-by-pair one returns,
and both equal the restatement on the CPU oracle (tests/lk_fb_ref.py)."""
import os
import subprocess

import numpy as np
import pytest

import lk_fb_ref as F
import lk_window_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    exe = tmp_path_factory.mktemp("lk_fb_mirror") / "lk_fb_mirror.bin"
    pk = os.path.join(ROOT, "visual-odometry-gpu_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(pk, "host"), "-o",
                           str(exe), os.path.join(ROOT, "tests", "cpp", "lk_fb_mirror.cpp"), "-L" + pk, "-lorbx",
                           "-Wl,-rpath," + pk, "-Wl,-rpath,/opt/rocm/lib"])
    return str(exe)


def run(mirror, mode, path, thr):
    r = subprocess.run([mirror, mode, str(path), repr(thr)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_one_launch_equals_pair_by_pair(mirror, tmp_path):
    frames = R.shifted_frames(2, 96, 128, 5, (-6.5, 4.0))
    pts = R.box_points(2, 300, 96, 128)
    path = tmp_path / "window.bin"
    path.write_bytes(np.int32([5, 128, 96]).tobytes() + frames.tobytes() + np.int32(len(pts)).tobytes() + pts.tobytes())
    pairs, launch = run(mirror, "pairs", path, 1.0), run(mirror, "launch", path, 1.0)
    assert launch == pairs
    # and both are the restatement's tracks
    tracks, seen, _, _, lost = F.track_window(frames, pts, 1.0, **R.REFERENCE)
    assert F.reasons(lost) == [57, 158, 8, 77]
    lines = launch.splitlines()
    assert len(lines) == 300
    for i, ln in enumerate(lines):
        tok = ln.split()
        assert int(tok[0]) == seen[i] and int(tok[1]) == lost[i]
        obs = np.array([float.fromhex(v) for v in tok[2:]]).reshape(-1, 3)
        assert np.array_equal(obs[:, 0], np.arange(seen[i]))
        assert np.array_equal(obs[:, 1:].astype(np.float32).view(np.uint32), tracks[i, :seen[i]].view(np.uint32))
