"""CPU-only checks of the fourth public header, include/orbx_stream.h, against the binding's fourth prototype table
(orbx_stream.PROTOTYPES), the way tests/test_orbx_lm_abi.py pins include/orbx_lm.h to orbx_lm.PROTOTYPES: every
function declared with the header's parameter classes, the view structure and the status bits with the header's, the
prototypes applied in one place, every symbol exported by liborbx.so, every declaration citing the reference -- and,
without a GPU, the entries refusing as the others do.  The first three headers and tables stay as they were: nothing
of rank 16 is in them.  Also here: the layouts of the stitch's blocks against their formulas
(tests/cpp/st_layout_pins.cpp)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

from test_binding_prototypes import RETURNS, SCALARS, is_pointer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("orbx_window_poses_stream_device", "orbx_stitch_windows_device", "orbx_stitch_results_device",
           "orbx_stitch_fetch", "orbx_stitch_windows", "orbx_stream_odometry_tracks_device",
           "orbx_stream_odometry_tracks")
CITE_FILE, CITE_LINES = "src/with_bundle_adjustment.cpp:", (":203", ":234-249")


def raw_header(name="orbx_stream.h"):
    return open(os.path.join(ROOT, "include", name)).read()


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
    table, decls = pkg.orbx_stream.PROTOTYPES, declarations()
    assert sorted(decls) == sorted(table) == sorted(ENTRIES) and pkg.orbx_stream.EXPORTS == list(table)
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
        assert params[-1] == "void* stream" or not name.endswith("_device") or name == "orbx_stitch_results_device"


def test_the_stream_entries_share_their_arguments(pkg):
    """the host twin takes the device entry's arguments without the stream, then its five outputs; both take the
    options of orbx_window_odometry_tracks (prob .. max_trans) around the two of the views build"""
    dev = pkg.orbx_stream.PROTOTYPES["orbx_stream_odometry_tracks_device"]
    host = pkg.orbx_stream.PROTOTYPES["orbx_stream_odometry_tracks"]
    assert host[0] is dev[0] and host[1] == dev[1][:-1] + [C.c_void_p] * 5
    d = declarations()
    names = lambda n: [p.split()[-1].lstrip("*") for p in d[n][1]]
    assert names("orbx_stream_odometry_tracks")[:len(dev[1]) - 1] == \
        [n.replace("d_tracks_xy", "tracks_xy").replace("d_seen", "seen").replace("slot_capacity", "n_slots")
         for n in names("orbx_stream_odometry_tracks_device")[:-1]]
    chain = pkg.orbx_vo.PROTOTYPES["orbx_window_poses_device"]
    assert pkg.orbx_stream.PROTOTYPES["orbx_window_poses_stream_device"][1] == \
        [chain[1][0], C.c_int, C.c_double, chain[1][-1]]


def test_view_and_status_bits_against_header(pkg):
    o = pkg.orbx_stream
    views = re.findall(r"typedef\s+struct\s*\{([^}]*)\}\s*orbx_(\w+)_view\s*;", header())
    assert [n for _, n in views] == ["stitch"]
    want = []
    for decl in filter(None, (" ".join(d.split()) for d in views[0][0].split(";"))):
        pointer = "*" in decl
        ctype = " ".join(w for w in decl.split(",")[0].split()[:-1] if w != "const")
        assert pointer or ctype == "int32_t", "field %r is neither a pointer nor int32_t" % decl
        want += [(field.replace("*", " ").split()[-1], pointer) for field in decl.split(",")]
    assert [(f, is_pointer(t)) for f, t in o.StitchView._fields_] == want
    assert [f for f, _ in want] == ["trajectory4x4", "owner", "anchors4x4", "lambda", "status", "n_frames",
                                    "n_windows", "window_len", "stride"]
    assert all(t is C.c_int32 for _, t in o.StitchView._fields_ if not is_pointer(t))
    assert C.sizeof(o.StitchView) == 5 * 8 + 4 * 4
    enums = dict((n, int(v)) for n, v in re.findall(r"\b(ORBX_ST_[A-Z_]+)\s*=\s*(\d+)", header()))
    assert enums == dict(ORBX_ST_OK=o.ST_OK, ORBX_ST_BROKEN=o.ST_BROKEN,
                         ORBX_ST_SCALE_UNALIGNED=o.ST_SCALE_UNALIGNED)
    assert sorted(enums.values()) == [0, 1, 2]


def test_the_four_headers_and_tables_do_not_overlap(pkg):
    others = [raw_header(h) for h in ("orbx.h", "orbx_vo.h", "orbx_lm.h")]
    modules = (pkg.orbx, pkg.orbx_vo, pkg.orbx_lm, pkg.orbx_stream)
    for name in ENTRIES:
        assert all(name not in src for src in others), name
        assert all(name not in m.PROTOTYPES for m in modules[:3]), name
    tables = [set(m.PROTOTYPES) for m in modules]
    for i in range(4):
        for j in range(i + 1, 4):
            assert not (tables[i] & tables[j]), (i, j)
    assert '#include "orbx.h"' in raw_header() and "orbx_vo.h\"" not in header() and "orbx_lm.h\"" not in header()
    assert pkg.orbx_stream.load() is pkg.orbx.load()


def test_prototypes_are_set_in_load_and_nowhere_else(pkg):
    o = pkg.orbx_stream
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
    for name in ENTRIES:
        at = src.index("int %s(" % name)
        comment = src[:at].rsplit("/*", 1)[1]
        assert CITE_FILE in comment and any(c in comment for c in CITE_LINES), name
    at = src.index("} orbx_stitch_view;")
    comment = src[:at].rsplit("/* Device-side view", 1)[1]
    assert CITE_FILE in comment and CITE_LINES[1] in comment


def test_the_functions_take_a_context(pkg):
    for f in ("window_poses_stream", "stitch_windows_device", "stitch_view", "stitch_fetch",
              "stream_odometry_tracks_device", "stream_odometry_tracks"):
        assert list(inspect.signature(getattr(pkg.orbx_stream, f)).parameters)[0] == "ctx", f
    assert list(inspect.signature(pkg.orbx_stream.stitch_windows).parameters)[0] == "poses"  # host only: no context
    src = inspect.getsource(pkg.orbx_stream)
    assert "_tracks_args(" in src and "_stream(" in src and "_device_arg(" in src  # arguments through orbx's helpers
    assert pkg.orbx_stream is __import__("importlib").import_module(pkg.__name__ + ".orbx_stream")


def test_without_a_context_the_entries_refuse(pkg):
    """a NULL context is ORBX_ERR_INVALID_ARG before anything touches a device, as for every entry of the other
    headers"""
    lib = pkg.orbx_stream.load()
    K = np.eye(3)
    bad = pkg.orbx.ERR_INVALID_ARG
    assert lib.orbx_window_poses_stream_device(None, 1, 1.0, None) == bad
    assert lib.orbx_stitch_windows_device(None, None, 2, 3, 1, None, 0, None) == bad
    assert lib.orbx_stitch_results_device(None, None) == bad
    assert lib.orbx_stitch_fetch(None, 0, 1, None, None, 0, 1, None, None, None) == bad
    options = (None, 1.0, 0.999, 1.0, 10, 0, 0, 0.0, 1.0, 10, 0.5, 50.0, 0)
    assert lib.orbx_stream_odometry_tracks_device(None, K.ctypes.data, None, None, 2, 4, 3, 1, *options, None) == bad
    assert lib.orbx_stream_odometry_tracks(None, K.ctypes.data, None, None, 2, 4, 3, 1, *options, None, None, None,
                                           None, None) == bad


def test_block_layout(tmp_path):
    exe = tmp_path / "st_layout_pins.bin"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(rocm, "include"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "st_layout_pins.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    m = re.search(r"(\d+) values compared, (\d+) failures", r.stdout)
    assert m and int(m.group(2)) == 0 and int(m.group(1)) == 256 * 28 * 12
