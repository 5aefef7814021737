"""The tables of a frame size for EVERY NMS radius, on the host (no GPU): tests/cpp/tile_tables_radius_sweep.cpp calls
build_tile_tables (csrc/orbx_tables.h) under AddressSanitizer and UBSan with nms_window 0, 3, 5 and 7 (R = 0 .. 3),
both FAST kernels, first passes of 0, 1 and 2 tile rows, fresh / learned / chosen / forced cuts, on the frame sizes of
plan_tables_replay.cpp and on 320 x 160, and asserts properties instead of hashes --

1. the first pyramid pass reaches every row its FAST units read (R + 3 rows below the end D of the first-pass tile
   rows); without an early band it ends at D + ORBX_TOP_MARGIN, with one at P >= max(D + R + 3, h0 + ORBX_TOP_MARGIN)
   and the band's strips, tested on tile row 0 alone, cover [P, D + ORBX_TOP_MARGIN);
2. the strips of the two passes together cover every row of every strip column exactly once;
3. the FAST units of a level tile its rows exactly once, none taller than fast_unit_rows_max, first-pass units first;
4. mask_wpr, mask_strip_px and the strips in x cover the level's width, each strip's ring and NMS context inside the
   256 pixels it loads.

(A halo of R + 2 instead of R + 3 in pyrblur_early_rows makes 1. fail: tried on a scratch copy.)"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_radius_kernel_and_cut_gives_tables_the_kernels_can_rely_on(tmp_path):
    exe = tmp_path / "tile_tables_radius_sweep.bin"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "tile_tables_radius_sweep.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and not r.stderr, r.stdout[-3000:] + r.stderr[-3000:]
    assert "0 failures" in r.stdout and "FAIL" not in r.stdout
    # the sweep really swept: 6 sizes x 3 scales x 4 radii x 2 kernels x 3 first passes x 18 states
    m = re.search(r"(\d+) cases: levels with two passes (\d+), with one (\d+), with a cut (\d+) \((\d+) moved to a legal one\), "
                  r"with an early band (\d+)", r.stdout)
    assert m, r.stdout[-1000:]
    cases, two, one, cut, moved, band = map(int, m.groups())
    assert cases == 6 * 3 * 4 * 2 * 3 * 18
    assert min(two, one, cut, moved, band) > 100
