"""Shapes of the k_pyrblur tests (tests/test_pyrblur_bands.py, tests/test_cpp_pyrblur_bands.py) and the host program
that tells, through the library's own table builders (csrc/orbx_plan.h), which bands they give."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pyrblur_bands_mirror.cpp")
NLEVELS, TOP_ROWS = 8, 2  # (ORBX_TOP_ROWS' default: the first pass holds two FAST tile rows)

# name: frame width, height, scale factor.  Three FAST tile rows at level 0, so the pyramid is built in two passes; the
# first pass cuts the lower levels' strips into two bands (a band that starts below row 0 begins without a carried
# source row although the row above it exists) and leaves the upper levels one band each.  506 px: the third strip
# of level 0 holds two dwords, the second of them half a dword.  Scale 1.1: seven levels resized through the 8-byte
# window, most of whose rows share a source row with the row above; 1.41: two such levels, the second (x1.99) with
# hardly any shared row, and the upper levels on the staged and the gather paths.
CASES = {
    "s12-500x134": dict(w=500, h=134, scale=1.2),
    "s12-506x126": dict(w=506, h=126, scale=1.2),
    "s11-500x114": dict(w=500, h=114, scale=1.1),
    "s141-500x119": dict(w=500, h=119, scale=1.41),
}


def compile_mirror(out, sanitize):
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-o", str(out), SRC])
    return str(out)


def band_table(exe, case):
    """{'whole': entries of the every-row table, 'tile_rows': FAST tile rows of level 0,
    'levels': [(w, h, first-pass rows, [band heights])]}"""
    r = subprocess.run([exe, "bands", str(case["w"]), str(case["h"]), repr(case["scale"]), str(NLEVELS), str(TOP_ROWS)],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    out = dict(levels=[])
    for ln in r.stdout.splitlines():
        tok = ln.split()
        if tok[0] == "whole":
            out["whole"] = int(tok[1])
        elif tok[0] == "fast_tile_rows":
            out["tile_rows"] = int(tok[1])
        elif tok[0] == "level":
            assert int(tok[1]) == len(out["levels"])
            out["levels"].append((int(tok[2]), int(tok[3]), int(tok[4]), [int(v) for v in tok[5:]]))
    assert len(out["levels"]) == NLEVELS
    return out


def check_shapes(exe):
    """the chosen sizes give the tables they were chosen for; returns {name: band_table}"""
    tables, seen = {}, set()
    for name, case in CASES.items():
        t = tables[name] = band_table(exe, case)
        assert t["tile_rows"] >= 3, (name, t)  # or there is no second pass at all
        nbands = []
        for w, h, first, bands in t["levels"]:
            assert sum(bands) == first <= h and max(bands) <= 58, (name, t)
            nbands.append(len(bands))
        assert t["levels"][0][2] < t["levels"][0][1], (name, t)  # level 0 has rows left for the second pass
        assert 2 in nbands, (name, nbands)  # strips of two bands ...
        seen |= set(nbands)
    assert seen == {1, 2}, seen  # ... and of one
    return tables
