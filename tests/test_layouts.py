"""Every block layout of the host layer is what it was before csrc/orbx_layout.h gathered them (host only).

Where the sections of a result block, a workspace or a scratch buffer lie, how large the block is, and how many frames
a workspace holds decide what the kernels are handed and how many launches a call makes.  tests/cpp/layout_pins.cpp
restates the formulas as they stood in orbx_api_gftt.cpp, orbx_api_lk.cpp, orbx_api_landmarks.cpp, orbx_api_tracks.cpp
and orbx_host.h -- the align_up_sz chains written out -- and compares every offset, total and frames-per-slice value
with the header's over n in {1 .. 256}, frames from 8 x 8 to 1920 x 1080, 1 .. 2000 slots, windows of 2, 3 and 8 frames,
the grid strides of min_distance 0, 1, 2 and 8, workspace limits from less than one frame's worth up to the defaults,
and LK windows 3, 21, 31 with up to 0, 3, 7 levels above the first.

The blocks of matcher, pose, scale, bundle adjustment of staged windows and the pair tracker were one buffer per array
before: for them the program writes out the chain of those buffers' byte counts, each rounded up to 256, over 1 .. 256
pairs of 1 .. 2000 slots, host entries of 0 .. 3000 points and windows of 2 .. 8 poses with 1 .. 65536 landmarks, and
checks that every section lies where the chain puts it, at a multiple of 256, and holds the earlier request; the
bundle-adjustment group count is the formula orbx_bundle_adjust_batch had."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pins(tmp_path_factory):
    """The program, compiled here with the host compiler alone (test infrastructure; not part of build())."""
    out = tmp_path_factory.mktemp("layout_pins") / "layout_pins.bin"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(rocm, "include"), "-o", str(out),
                           os.path.join(ROOT, "tests", "cpp", "layout_pins.cpp")])
    return str(out)


def test_every_layout_and_slice_is_the_previous_formula(pins):
    r = subprocess.run([pins], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    m = re.search(r"(\d+) values compared, (\d+) failures", r.stdout)
    assert m, r.stdout[-1000:]
    compared, failures = map(int, m.groups())
    assert failures == 0 and "FAIL" not in r.stdout
    assert compared > 112_000_000  # the sweep really swept
