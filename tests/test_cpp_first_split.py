"""The unevenly cut first pass of the FAST tile rows on the host (no GPU): tests/cpp/first_split_sweep.cpp runs the
library's own geometry and cost model (csrc/orbx_plan.h) under AddressSanitizer and UBSan --

* for every level height 8..400, several tile-row preferences, both FAST layouts and every pair of first-pass heights
  of the level's depth, the units cover every row exactly once, follow each other in band order, and the table fits
  fast_tiles_upper_bound; a pair the kernels cannot run is ignored;
* the first pass of the fused pyramid + blur reaches the last first-pass FAST row + ORBX_TOP_MARGIN;
* the chooser answers equal halves for an empty histogram, for fill rows concentrated at the depth and for caps that
  never fill, and the cuts worked out for levels 0 and 2 of the benchmark stream (68 of 80 rows, 61 of 70) with the
  constants they were worked out with."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_partition_bound_boundary_and_chooser(tmp_path):
    exe = tmp_path / "first_split_sweep.bin"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "first_split_sweep.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "0 failures" in r.stdout and "FAIL" not in r.stdout
    cases = int(r.stdout.split("partitions: ")[1].split()[0])
    assert cases > 300000  # the sweep really swept
