"""The early band of the fused pyramid + blur kernel's second pass on the host (no GPU):
tests/cpp/pyramid_early_band_sweep.cpp runs the library's own table builder, boundary and rule (csrc/orbx_plan.h)
under AddressSanitizer and UBSan --

* for every level height 8..400, NMS radius 1 and 3, both FAST layouts, several tile-row preferences and every legal
  pair of first-pass heights: the first pass, the band and the rest cover every row exactly once; the first pass
  reaches h0 + ORBX_TOP_MARGIN and the last row a first-launch FAST unit reads; the band's strips test tile row 0
  alone and never report, the rest tests both tile rows; the second-pass table fits the pool bound; and without the
  new argument the tables equal, entry for entry, what the builder made before the band existed;
* the rule that applies the band per level: all frames leave, none leave, an empty histogram, a band of a row or two,
  shares between, and the buckets' conservative answer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tables_bound_boundary_and_rule(tmp_path):
    exe = tmp_path / "pyramid_early_band_sweep.bin"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "pyramid_early_band_sweep.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "0 failures" in r.stdout and "FAIL" not in r.stdout
    cases = int(r.stdout.split("tables: ")[1].split()[0])
    bands = int(r.stdout.split("cases, ")[1].split()[0])
    assert cases > 100000 and bands > 50000  # the sweep really swept, and met bands
