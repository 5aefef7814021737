"""The tile pools hold every frame the context accepts (host only; ADVICE.md, first finding).

A context allocates its table pools once, from max_width x max_height, and builds the tables of every frame size it
is given into them.  tests/cpp/plan_capacity_sweep.cpp runs the library's own geometry (csrc/orbx_plan.h) over
maxima x frames x tile-row preferences x both FAST layouts x 8 / 12 levels x scale 1.2 / 1.5 x NMS window 3 / 7 and
checks every table and pool against the capacity the maximum provides.  The second test puts the FAST pool's sizing
back to what it was before the upper bound and expects the sweep to report the frame that then overflows."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    """The sweep program, compiled here (test infrastructure; not part of build())."""
    out = tmp_path_factory.mktemp("plan_sweep") / "plan_capacity_sweep.bin"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-pthread", "-o", str(out),
                           os.path.join(ROOT, "tests", "cpp", "plan_capacity_sweep.cpp")])
    return str(out)


def test_every_accepted_frame_fits_the_pools_of_its_maximum(sweep):
    r = subprocess.run([sweep], capture_output=True, text=True, timeout=1800)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    m = re.search(r"(\d+) \(maximum, configuration\) pairs \((\d+) not creatable\), (\d+) frames \((\d+) refused "
                  r"whatever the maximum\), (\d+) \(maximum, frame, preference\) triples, (\d+) failures", r.stdout)
    assert m, r.stdout[-1000:]
    pairs, uncreatable, frames, refused, triples, failures = map(int, m.groups())
    assert failures == 0 and "FAIL" not in r.stdout
    # the sweep really swept: 6 named + 200 random maxima x 16 configurations, most of them creatable, ~900 frames
    # each, few of them refused, ~40 preferences per frame
    assert pairs == 206 * 16 and uncreatable < pairs // 2
    assert frames > 800 * (pairs - uncreatable) and refused < frames // 20
    assert triples > 30 * (frames - refused)


def test_the_sweep_fails_on_the_previous_sizing_of_the_fast_pool(sweep):
    """The FAST pool sized as the table of the maximum itself with ORBX_MIN_TILE_H preferred on every level (the
    sizing before fast_tiles_upper_bound): a 594 x 1084 frame in a 600 x 1100 context needs 618 entries of 617, and
    2187 x 2084 in 2191 x 2141 needs 2642 of 2639 -- the sweep must say so."""
    r = subprocess.run([sweep, "--parent-sizing", "--maxima", "0"], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 1, r.stdout[-3000:] + r.stderr[-1000:]
    assert ("FAIL fast_impl=4 nlevels=8 scale=1.2 nms=3 max=600x1100 frame=594x1084 pref=[16,16,16,16,16,16,16,16]: "
            "FAST tile table needs 618, pool holds 617") in r.stdout
    assert re.search(r"max=2191x2141 frame=2187x2084 pref=\[16(,16){7}\]: FAST tile table needs 2642, pool holds 2639",
                     r.stdout)
