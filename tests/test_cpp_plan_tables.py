"""The tables of a frame size on the host (no GPU): tests/cpp/plan_tables_replay.cpp calls the two functions set_plan
calls (csrc/orbx_tables.h: plan_with_taps, build_tile_tables) under AddressSanitizer and UBSan --

* 7920 cases: 1241 x 376, 1920 x 1080, 160 x 160 (one tile row on the upper levels), 645 x 487 (odd, the width no
  multiple of 4) and 27 x 27 (the smallest size the library accepts, found by a scan from 8 x 8); scale factors 1.2,
  1.5 and 2.0, under which levels resize in each of the three modes (win8 0, 1, 3); both FAST layouts, the three blur
  kernels, strips grouped or not, first passes of 0 to 3 tile rows; and every state of the scheduler's record that
  changes a table: fresh, learned tile rows (with and without the pipeline), a chosen cut, forced cuts, 2:equal,
  2:late, histograms under which an early band pays and under which it does not.  Each case folds the levels' win8,
  the tap table, the blur tile map, the band map, every tile table, the levels the second pass may skip and the rows
  the first pass ends at into one hash per frame size.  The expected hashes were recorded from set_plan as it stood
  inside orbx_api.cpp before the sequence moved into the header;
* scripted: learned tile rows that need one entry more than the FAST pool holds are forgotten and the tables are those
  of a fresh record; every table whose pool is one entry short is refused with its message."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_table_bytes_of_every_case_and_the_refusals(tmp_path):
    exe = tmp_path / "plan_tables_replay.bin"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "plan_tables_replay.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "0 failures" in r.stdout and "FAIL" not in r.stdout
    replays = [line for line in r.stdout.splitlines() if line.startswith("replay ")]
    assert len(replays) == 5 and "scripted: hash" in r.stdout  # the replay really ran
    assert "7920 cases" in r.stdout
