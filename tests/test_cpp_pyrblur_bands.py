"""Row bookkeeping of k_pyrblur on the host (no GPU): tests/cpp/pyrblur_bands_mirror.cpp restates how the kernel finds
the y tap of a band's input row (one per lane) and its "same source row as the row above" flag (equality of the CLAMPED
source indices, carried from request to request) and compares both with a per-row computation, for every level of
every frame height 8 .. 400 at scales 1.1, 1.2 and 1.41, over the strip tables csrc/orbx_plan.h builds.  Stand-alone
program, built with -fsanitize=address,undefined.  And the shapes of tests/test_pyrblur_bands.py give the tables they
were chosen for."""
import re

import pytest

import pyrblur_cases as PC


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    return PC.compile_mirror(tmp_path_factory.mktemp("pyrblur_bands") / "pyrblur_bands_mirror.bin", sanitize=True)


def test_tap_lanes_and_reuse_flag_equal_the_per_row_computation(mirror):
    import subprocess

    r = subprocess.run([mirror, "sweep"], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "FAIL" not in r.stdout and not r.stderr, r.stdout[-3000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) bands, (\d+) row requests, (\d+) failures", r.stdout)
    assert m, r.stdout[-1000:]
    bands, requests, failures = map(int, m.groups())
    assert failures == 0
    # the sweep really swept: three scales x 393 heights x (up to) 7 resized levels x three tables
    assert bands > 30000 and requests > 40 * bands
    # scale <= 2 levels at every scale, mostly-shared and rarely-shared rows among them
    shares = [float(v) for v in re.findall(r"\(([\d.]+) %\)", r.stdout)]
    assert len(shares) >= 12 and max(shares) > 80 and min(shares) < 5


def test_the_shapes_of_the_gpu_tests_give_the_tables_they_were_chosen_for(mirror):
    tables = PC.check_shapes(mirror)
    for name, t in tables.items():
        assert -(-4096 // t["whole"]) <= 256, (name, t["whole"])  # batches of a few hundred small frames
