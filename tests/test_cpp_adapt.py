"""The scheduler of the first pass on the host (no GPU): tests/cpp/adapt_replay.cpp replays batches through the
library's own steps (csrc/orbx_adapt.h) under AddressSanitizer and UBSan, rebuilding the tables after every re-tile
with the builder set_plan calls (csrc/orbx_tables.h: build_tile_tables), on 1241 x 376 (both FAST layouts) and on 160 x 160, whose upper levels have one tile row --

* scripted streams with the value every rule gives: observation windows of 2, 4, 8, 16, 32, 32 batches that an
  all-zero batch does not advance; grow at once, shrink only for three rows, settle after four re-tiles; whole groups
  of 7 rows for the streaming kernel; the cut of the first pass chosen, moved for 1000 milli-groups, withdrawn, voided
  by new heights, forced and clamped at both ends; early bands split, kept, forced and switched off; the adaptive
  verdict with its probe and wrapping counters; the reset on a new frame size; the fields behind ORBX_TOP_ROWS' number;
  the three trace lines byte for byte;
* a seeded stream of 20000 batches per geometry whose every step is folded into a hash.  The expected hashes were
  recorded from the scheduler as it stood inside orbx_api.cpp before it moved into the header."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scripted_streams_and_seeded_replay(tmp_path):
    exe = tmp_path / "adapt_replay.bin"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "adapt_replay.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "0 failures" in r.stdout and "FAIL" not in r.stdout
    seeded = [line for line in r.stdout.splitlines() if line.startswith("seeded ")]
    assert len(seeded) == 3  # the replay really ran
    assert all(int(line.split(", ")[1].split()[0]) >= 100 for line in seeded)  # and the streams made the tables change
