"""CPU-only checks of the third public header, include/orbx_lm.h, against the binding's third prototype table
(orbx_lm.PROTOTYPES), the way tests/test_orbx_vo_abi.py pins include/orbx_vo.h to orbx_vo.PROTOTYPES: every function
declared with the header's parameter classes, the view structure with the header's fields, the prototypes applied in
one place, every symbol exported by liborbx.so, every declaration citing the reference -- and, without a GPU, the
entries refusing as the others do.  The first two headers and tables stay as they were: nothing of rank 15 is in them.
Also here: the layout of the views buffer against its formula (tests/cpp/lm_views_layout_pins.cpp)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

from test_binding_prototypes import RETURNS, SCALARS, is_pointer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("orbx_landmarks_build_views_device", "orbx_landmarks_views_results_device", "orbx_landmarks_views_fetch",
           "orbx_bundle_adjust_tracks_views")
CITE = "src/with_bundle_adjustment.cpp:502-575"


def raw_header(name="orbx_lm.h"):
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
    table, decls = pkg.orbx_lm.PROTOTYPES, declarations()
    assert sorted(decls) == sorted(table) == sorted(ENTRIES) and pkg.orbx_lm.EXPORTS == list(table)
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


def test_the_tracks_entry_extends_the_one_of_the_first_header(pkg):
    """orbx_bundle_adjust_tracks_views: orbx_bundle_adjust_tracks's arguments, then the two options"""
    base = pkg.orbx.PROTOTYPES["orbx_bundle_adjust_tracks"]
    ext = pkg.orbx_lm.PROTOTYPES["orbx_bundle_adjust_tracks_views"]
    assert ext[0] is base[0] and ext[1] == base[1] + [C.c_int, C.c_double]
    build = pkg.orbx.PROTOTYPES["orbx_landmarks_build_device"]
    views = pkg.orbx_lm.PROTOTYPES["orbx_landmarks_build_views_device"]
    assert views[1] == build[1][:-1] + [C.c_int, C.c_double] + build[1][-1:]  # (the stream stays last)


def test_view_and_enums_against_header(pkg):
    o = pkg.orbx_lm
    views = re.findall(r"typedef\s+struct\s*\{([^}]*)\}\s*orbx_(\w+)_view\s*;", header())
    assert [n for _, n in views] == ["landmarks_views"]
    body = views[0][0]
    want = []
    for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
        pointer = "*" in decl
        ctype = " ".join(w for w in decl.split(",")[0].split()[:-1] if w != "const")
        assert pointer or ctype == "int32_t", "field %r is neither a pointer nor int32_t" % decl
        want += [(field.replace("*", " ").split()[-1], pointer) for field in decl.split(",")]
    assert [(f, is_pointer(t)) for f, t in o.LandmarksViewsView._fields_] == want
    assert all(t is C.c_int32 for _, t in o.LandmarksViewsView._fields_ if not is_pointer(t))
    assert C.sizeof(o.LandmarksViewsView) == 2 * 8 + 2 * 4
    enums = dict((n, int(v)) for n, v in re.findall(r"\b(ORBX_LM_[A-Z_]+)\s*=\s*(\d+)", header()))
    assert enums == dict(ORBX_LM_TRI_FIRST_TWO=o.TRI_FIRST_TWO, ORBX_LM_TRI_WIDEST=o.TRI_WIDEST,
                         ORBX_LM_TRI_ALL_VIEWS=o.TRI_ALL_VIEWS, ORBX_LM_KEPT=o.KEPT, ORBX_LM_SHORT=o.SHORT,
                         ORBX_LM_DEGENERATE=o.DEGENERATE, ORBX_LM_BEHIND=o.BEHIND,
                         ORBX_LM_REPROJECTION=o.REPROJECTION, ORBX_LM_NO_WINDOW=o.NO_WINDOW)
    assert sorted(enums.values()) == [0, 0, 1, 1, 2, 2, 3, 4, 5]


def test_the_three_headers_and_tables_do_not_overlap(pkg):
    first, second = raw_header("orbx.h"), raw_header("orbx_vo.h")
    for name in ENTRIES:
        assert name not in first and name not in second, name
        assert name not in pkg.orbx.PROTOTYPES and name not in pkg.orbx_vo.PROTOTYPES, name
    tables = [set(m.PROTOTYPES) for m in (pkg.orbx, pkg.orbx_vo, pkg.orbx_lm)]
    assert not (tables[0] & tables[1]) and not (tables[0] & tables[2]) and not (tables[1] & tables[2])
    assert '#include "orbx.h"' in raw_header() and "orbx_vo.h\"" not in header()
    assert pkg.orbx_lm.load() is pkg.orbx.load()


def test_prototypes_are_set_in_load_and_nowhere_else(pkg):
    o = pkg.orbx_lm
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
        assert CITE in comment, name
    at = src.index("} orbx_landmarks_views_view;")
    assert CITE in src[:at].rsplit("/* Device-side view", 1)[1]


def test_the_functions_take_a_context(pkg):
    for f in ("landmarks_build_views", "landmarks_views_view", "landmarks_views_fetch", "bundle_adjust_tracks_views"):
        assert list(inspect.signature(getattr(pkg.orbx_lm, f)).parameters)[0] == "ctx", f
    src = inspect.getsource(pkg.orbx_lm)
    assert "_tracks_args(" in src and "_stream(" in src and "_host_window(" in src  # arguments through orbx's helpers


def test_without_a_context_the_entries_refuse(pkg):
    """a NULL context is ORBX_ERR_INVALID_ARG before anything touches a device, as for every entry of the other
    headers"""
    lib = pkg.orbx_lm.load()
    K = np.eye(3)
    assert lib.orbx_landmarks_build_views_device(None, K.ctypes.data, None, None, 1, 1, 2, None, 2, 3.0, None) == \
        pkg.orbx.ERR_INVALID_ARG
    assert lib.orbx_landmarks_views_results_device(None, None) == pkg.orbx.ERR_INVALID_ARG
    assert lib.orbx_landmarks_views_fetch(None, 0, 1, None, None) == pkg.orbx.ERR_INVALID_ARG
    assert lib.orbx_bundle_adjust_tracks_views(None, K.ctypes.data, None, None, 1, 2, None, 1.0, 10, None, None, None,
                                               None, 0, None, 2, 3.0) == pkg.orbx.ERR_INVALID_ARG


def test_block_layout(tmp_path):
    exe = tmp_path / "lm_views_layout_pins.bin"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(rocm, "include"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "lm_views_layout_pins.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    m = re.search(r"(\d+) values compared, (\d+) failures", r.stdout)
    assert m and int(m.group(2)) == 0 and int(m.group(1)) == 256 * 7 * 9 * 5
