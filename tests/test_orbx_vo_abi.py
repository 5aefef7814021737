"""CPU-only checks of the second public header, include/orbx_vo.h, against the binding's second prototype table
(orbx_vo.PROTOTYPES), the way tests/test_binding_prototypes.py pins include/orbx.h to orbx.PROTOTYPES: every function
declared with the header's parameter classes, the *View structures with the header's fields, the prototypes applied in
one place, every symbol exported by liborbx.so, every declaration citing the reference -- and, without a GPU, the
device entries refusing as the others do.  The first header and table stay as they were: nothing of rank 14 is in them.
Also here: the layouts of the path's three blocks against their formulas (tests/cpp/wp_layout_pins.cpp)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from test_binding_prototypes import RETURNS, SCALARS, is_pointer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("orbx_window_poses_device", "orbx_window_poses_results_device", "orbx_window_poses_fetch",
           "orbx_chain_window_poses", "orbx_landmarks_build_chained_device", "orbx_bundle_adjust_write_back_device",
           "orbx_bundle_adjust_write_back_results_device", "orbx_bundle_adjust_write_back_fetch",
           "orbx_window_odometry_tracks")
CITES = ("src/with_bundle_adjustment.cpp:196-208", "src/with_bundle_adjustment.cpp:615-628",
         "src/with_bundle_adjustment.cpp:683-718")


def raw_header():
    return open(os.path.join(ROOT, "include", "orbx_vo.h")).read()


def header():
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", raw_header(), flags=re.S))


def declarations():
    src = header()
    out = {}
    for ret, name, params in re.findall(r"^([A-Za-z_][\w \t\*]*?)\s*\b(orbx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        params = [" ".join(p.split()) for p in params.split(",")]
        out[name] = (re.sub(r"\s*\*", "*", " ".join(ret.split())), [] if params == ["void"] else params)
    assert sorted(out) == sorted(set(re.findall(r"\b(orbx_[a-z0-9_]+)\s*\(", src)))  # no declaration slipped through
    return out


def test_table_against_header(pkg):
    table, decls = pkg.orbx_vo.PROTOTYPES, declarations()
    assert sorted(decls) == sorted(table) == sorted(ENTRIES) and pkg.orbx_vo.EXPORTS == list(table)
    for name, (ret, params) in decls.items():
        restype, argtypes = table[name]
        assert ret in RETURNS and restype is RETURNS[ret], name
        assert len(argtypes) == len(params), name
        for i, (p, got) in enumerate(zip(params, argtypes)):
            if "*" in p:
                assert is_pointer(got), (name, i, p)
                continue
            ctype = " ".join(w for w in p.split()[:-1] if w != "const")
            assert ctype in SCALARS, "%s, parameter %d: type %r is outside the header's vocabulary" % (name, i, p)
            assert got is SCALARS[ctype], (name, i, p)


def test_views_against_header(pkg):
    views = re.findall(r"typedef\s+struct\s*\{([^}]*)\}\s*orbx_(\w+)_view\s*;", header())
    assert sorted(n for _, n in views) == ["ba_write_back", "window_poses"]
    for body, name in views:
        struct = getattr(pkg.orbx_vo, "".join(w.capitalize() for w in name.split("_")) + "View")
        want = []
        for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
            pointer = "*" in decl
            ctype = " ".join(w for w in decl.split(",")[0].split()[:-1] if w != "const")
            assert pointer or ctype == "int32_t", "%s: field %r is neither a pointer nor int32_t" % (name, decl)
            want += [(field.replace("*", " ").split()[-1], pointer) for field in decl.split(",")]
        assert [(f, is_pointer(t)) for f, t in struct._fields_] == want, name
        assert all(t is C.c_int32 for _, t in struct._fields_ if not is_pointer(t)), name
    assert C.sizeof(pkg.orbx_vo.WindowPosesView) == 3 * 8 + 2 * 4 and C.sizeof(pkg.orbx_vo.BaWriteBackView) == 2 * 8 + 2 * 4


def test_the_two_headers_and_tables_do_not_overlap(pkg):
    first = open(os.path.join(ROOT, "include", "orbx.h")).read()
    for name in ENTRIES:
        assert name not in first and name not in pkg.orbx.PROTOTYPES, name
    assert '#include "orbx.h"' in raw_header()
    assert pkg.orbx_vo.load() is pkg.orbx.load()


def test_prototypes_are_set_in_load_and_nowhere_else(pkg):
    o = pkg.orbx_vo
    lib = o.load()
    for name, (restype, argtypes) in o.PROTOTYPES.items():
        f = getattr(lib, name)
        assert f.argtypes is not None and list(f.argtypes) == list(argtypes) and f.restype is restype, name
    src, applied = inspect.getsource(o), inspect.getsource(o.load)
    for pattern in (r"\.argtypes\s*=", r"\.restype\s*="):
        assert len(re.findall(pattern, src)) == len(re.findall(pattern, applied)) == 1, pattern
    assert "argtypes" not in src.replace(applied, "")


def test_library_exports_every_declared_symbol(pkg):
    lib = pkg.orbx.load()
    for name in declarations():
        assert hasattr(lib, name), name


def test_the_declarations_cite_the_reference():
    src = raw_header()
    for cite in CITES:
        assert cite in src, cite
    for name in ENTRIES:
        at = src.index("int %s(" % name)
        comment = src[:at].rsplit("/*", 1)[1]
        assert re.search(r"src/\w+\.cpp:\d+", comment), name
    for view in ("orbx_window_poses_view", "orbx_ba_write_back_view"):
        at = src.index("} %s;" % view)
        assert re.search(r"src/\w+\.cpp:\d+", src[:at].rsplit("/* Device-side view", 1)[1]), view


def test_the_functions_take_a_context(pkg):
    for f in ("window_poses", "window_poses_view", "window_poses_fetch", "landmarks_build_chained",
              "bundle_adjust_write_back", "bundle_adjust_write_back_view", "bundle_adjust_write_back_fetch",
              "window_odometry_tracks"):
        assert list(inspect.signature(getattr(pkg.orbx_vo, f)).parameters)[0] == "ctx", f
    assert list(inspect.signature(pkg.orbx_vo.chain_window_poses).parameters) == ["T0", "R", "t", "scale"]
    src = inspect.getsource(pkg.orbx_vo)
    assert "_tracks_args(" in src and "_stream(" in src  # device arguments through orbx's helpers


def test_without_a_context_the_device_entries_refuse(pkg):
    """a NULL context is ORBX_ERR_INVALID_ARG before anything touches a device, as for every entry of the first
    header; the host-only entry needs neither a context nor a GPU"""
    lib = pkg.orbx_vo.load()
    K = np.eye(3)
    assert lib.orbx_window_poses_device(None, None, None, None) == pkg.orbx.ERR_INVALID_ARG
    assert lib.orbx_window_poses_results_device(None, None) == pkg.orbx.ERR_INVALID_ARG
    assert lib.orbx_window_poses_fetch(None, 0, 1, None, None, None) == pkg.orbx.ERR_INVALID_ARG
    assert lib.orbx_landmarks_build_chained_device(None, K.ctypes.data, None, None, 1, 1, 2, None) == \
        pkg.orbx.ERR_INVALID_ARG
    assert lib.orbx_bundle_adjust_write_back_device(None, 0.5, 50.0, None) == pkg.orbx.ERR_INVALID_ARG
    assert lib.orbx_bundle_adjust_write_back_results_device(None, None) == pkg.orbx.ERR_INVALID_ARG
    assert lib.orbx_bundle_adjust_write_back_fetch(None, 0, 1, None, None) == pkg.orbx.ERR_INVALID_ARG
    assert lib.orbx_window_odometry_tracks(None, K.ctypes.data, None, None, 1, 2, None, 1.0, 0.999, 1.0, 10, 0, 1.0,
                                           10, 0.5, 50.0, None, None, None, None, None) == pkg.orbx.ERR_INVALID_ARG
    assert lib.orbx_chain_window_poses(None, None, None, None, -1, None, None) == pkg.orbx.ERR_INVALID_ARG
    p4, p6 = pkg.orbx_vo.chain_window_poses(None, np.eye(3)[None], [[0.0, 0.0, 1.0]], [2.0])
    assert np.array_equal(p4[1], [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -2.0], [0, 0, 0, 1]])
    assert np.array_equal(p6, [[0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 2.0]])


def test_block_layouts(tmp_path):
    exe = tmp_path / "wp_layout_pins.bin"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(rocm, "include"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "wp_layout_pins.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    m = re.search(r"(\d+) values compared, (\d+) failures", r.stdout)
    assert m and int(m.group(2)) == 0 and int(m.group(1)) == 1024 * 3 + 1024 * 7 * 7
