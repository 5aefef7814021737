"""CPU-only checks of the fifth public header, include/orbx_pnp.h, against the binding's fifth prototype table
(orbx_pnp.PROTOTYPES), the way tests/test_orbx_stream_abi.py pins include/orbx_stream.h: every function declared with
the header's parameter classes, the record and the view with the header's fields, the prototypes applied in one place,
every symbol exported by liborbx.so, every declaration citing the reference -- and, without a GPU, the entries refusing
as the others do.  The first four headers and tables stay as they were: nothing of rank 17 is in them.  Also here: the
record's offsets and the layouts of the two blocks against their formulas (tests/cpp/pnp_layout_pins.cpp)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

from test_binding_prototypes import RETURNS, SCALARS, is_pointer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("orbx_pnp_ransac", "orbx_window_poses_pnp_device", "orbx_window_poses_pnp_results_device",
           "orbx_window_poses_pnp_fetch", "orbx_window_poses_pnp_mask_fetch",
           "orbx_bundle_adjust_landmarks_pnp_device")
OTHER_HEADERS = ("orbx.h", "orbx_vo.h", "orbx_lm.h", "orbx_stream.h")
CITE = "src/with_bundle_adjustment.cpp:"


def raw_header(name="orbx_pnp.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def header(name="orbx_pnp.h"):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", raw_header(name), flags=re.S))


def declarations(name="orbx_pnp.h"):
    src = header(name)
    out = {}
    for ret, fn, params in re.findall(r"^([A-Za-z_][\w \t\*]*?)\s*\b(orbx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        params = [" ".join(p.split()) for p in params.split(",")]
        out[fn] = (re.sub(r"\s*\*", "*", " ".join(ret.split())), [] if params == ["void"] else params)
    assert sorted(out) == sorted(set(re.findall(r"\b(orbx_[a-z0-9_]+)\s*\(", src)))  # no declaration slipped through
    return out


def test_table_against_header(pkg):
    table, decls = pkg.orbx_pnp.PROTOTYPES, declarations()
    assert sorted(decls) == sorted(table) == sorted(ENTRIES) and pkg.orbx_pnp.EXPORTS == list(table)
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


def test_the_signatures_are_the_issued_ones():
    d = declarations()
    names = lambda fn: [p.replace("*", " ").split()[-1] for p in d[fn][1]]
    assert names("orbx_pnp_ransac") == ["ctx", "points3", "pixels_xy", "n", "K", "prob", "threshold_px", "max_iters",
                                        "seed", "refine_iters", "min_inliers", "pose6", "mask", "inliers", "iters",
                                        "rms_px", "status"]
    assert names("orbx_window_poses_pnp_device") == ["ctx", "prob", "threshold_px", "max_iters", "seed",
                                                     "refine_iters", "min_inliers", "stream"]
    assert names("orbx_bundle_adjust_landmarks_pnp_device") == ["ctx", "huber_delta", "max_iters", "stream"]
    assert names("orbx_window_poses_pnp_mask_fetch") == ["ctx", "window", "k", "mask", "capacity", "count"]
    assert names("orbx_window_poses_pnp_fetch")[:3] == ["ctx", "first", "n"]


def test_the_seeded_solve_extends_the_one_of_the_first_header(pkg):
    base = pkg.orbx.PROTOTYPES["orbx_bundle_adjust_landmarks_device"]
    assert pkg.orbx_pnp.PROTOTYPES["orbx_bundle_adjust_landmarks_pnp_device"] == base
    pose = pkg.orbx.PROTOTYPES["orbx_estimate_pose"][1]
    pnp = pkg.orbx_pnp.PROTOTYPES["orbx_pnp_ransac"][1]
    # K, prob, threshold, max_iters, seed: the classes of orbx_estimate_pose's
    assert pnp[4:9] == pose[4:9]


def struct_fields(body):
    want = []
    for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
        pointer = "*" in decl
        ctype = " ".join(w for w in decl.split(",")[0].split()[:-1] if w != "const")
        for field in decl.split(","):
            fname = field.replace("*", " ").split()[-1]
            m = re.match(r"(\w+)\[(\d+)\]", fname)
            want.append((m.group(1) if m else fname, pointer, ctype, int(m.group(2)) if m else 0))
    return want


def test_record_view_and_enums_against_header(pkg):
    o = pkg.orbx_pnp
    structs = dict((n, b) for b, n in re.findall(r"typedef\s+struct\s*\{([^}]*)\}\s*(orbx_\w+)\s*;", header()))
    assert sorted(structs) == ["orbx_pnp_record", "orbx_window_poses_pnp_view"]
    view = struct_fields(structs["orbx_window_poses_pnp_view"])
    assert [(f, is_pointer(t)) for f, t in o.WindowPosesPnpView._fields_] == [(f, p) for f, p, _, _ in view]
    assert all(p or c == "int32_t" for _, p, c, _ in view)
    assert all(t is C.c_int32 for _, t in o.WindowPosesPnpView._fields_ if not is_pointer(t))
    assert C.sizeof(o.WindowPosesPnpView) == 3 * 8 + 3 * 4 + 4
    rec = struct_fields(structs["orbx_pnp_record"])
    ctypes_of = {"double": C.c_double, "int32_t": C.c_int32}
    want = [(f, ctypes_of[c] * k if k else ctypes_of[c]) for f, _, c, k in rec]
    assert [(f, t._type_, getattr(t, "_length_", 0)) for f, t in o.PnpRecord._fields_] == \
        [(f, t._type_, getattr(t, "_length_", 0)) for f, t in want]
    assert C.sizeof(o.PnpRecord) == o.RECORD_DTYPE.itemsize == 72
    assert [(n, o.RECORD_DTYPE.fields[n][1]) for n in o.RECORD_DTYPE.names] == \
        [(f, getattr(o.PnpRecord, f).offset) for f, _ in o.PnpRecord._fields_]
    enums = dict((n, int(v)) for n, v in re.findall(r"\b(ORBX_PNP_[A-Z_]+)\s*=\s*(\d+)", header()))
    assert enums == dict(ORBX_PNP_OK=o.OK, ORBX_PNP_SKIPPED=o.SKIPPED, ORBX_PNP_FEW_POINTS=o.FEW_POINTS,
                         ORBX_PNP_NO_MODEL=o.NO_MODEL)
    assert sorted(enums.values()) == [0, 1, 2, 3]
    assert int(re.search(r"#define ORBX_PNP_MAX_REFINE_ITERS (\d+)", header()).group(1)) == o.MAX_REFINE_ITERS == 20


def test_no_symbol_of_the_other_four_headers_is_declared_again(pkg):
    mine = set(declarations())
    others = [pkg.orbx, pkg.orbx_vo, pkg.orbx_lm, pkg.orbx_stream]
    for name, mod in zip(OTHER_HEADERS, others):
        theirs = set(declarations(name))
        assert not (mine & theirs), (name, mine & theirs)
        assert not (set(pkg.orbx_pnp.PROTOTYPES) & set(mod.PROTOTYPES)), name
        for entry in ENTRIES:
            assert entry not in raw_header(name), (name, entry)
    assert len(declarations("orbx.h")) == 94  # the first header stays at its 94 declarations
    includes = re.findall(r'#include\s+"([^"]+)"', raw_header())
    assert includes == ["orbx.h"]  # the fifth header includes the first one only
    assert pkg.orbx_pnp.load() is pkg.orbx.load()


def test_prototypes_are_set_in_load_and_nowhere_else(pkg):
    o = pkg.orbx_pnp
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
    import __graft_entry__
    assert "orbx_pnp.EXPORTS" in inspect.getsource(__graft_entry__.build)


def test_the_declarations_cite_the_reference():
    src = raw_header()
    for name in ENTRIES:
        at = src.index("int %s(" % name)
        comment = src[:at].rsplit("/*", 1)[1]
        assert CITE in comment, name
    for struct in ("orbx_pnp_record", "orbx_window_poses_pnp_view"):
        at = src.index("} %s;" % struct)
        assert CITE in src[:at].rsplit("typedef struct", 1)[0].rsplit("/*", 1)[1], struct


def test_the_functions_take_a_context(pkg):
    for f in ("pnp_ransac", "window_poses_pnp", "window_poses_pnp_view", "window_poses_pnp_fetch",
              "window_poses_pnp_mask", "bundle_adjust_landmarks_pnp"):
        assert list(inspect.signature(getattr(pkg.orbx_pnp, f)).parameters)[0] == "ctx", f
    src = inspect.getsource(pkg.orbx_pnp)
    assert "_f64(" in src and "_stream(" in src and "_count(" in src  # arguments through orbx's helpers


def test_without_a_context_the_entries_refuse(pkg):
    """a NULL context is ORBX_ERR_INVALID_ARG before anything touches a device, as for every entry of the other
    headers"""
    lib = pkg.orbx_pnp.load()
    K = np.eye(3)
    bad = pkg.orbx.ERR_INVALID_ARG
    assert lib.orbx_pnp_ransac(None, None, None, 0, K.ctypes.data, 0.99, 2.0, 10, 0, 10, 4, None, None, None, None,
                               None, None) == bad
    assert lib.orbx_window_poses_pnp_device(None, 0.99, 2.0, 10, 0, 10, 4, None) == bad
    assert lib.orbx_window_poses_pnp_results_device(None, None) == bad
    assert lib.orbx_window_poses_pnp_fetch(None, 0, 1, None, None) == bad
    assert lib.orbx_window_poses_pnp_mask_fetch(None, 0, 2, None, 0, None) == bad
    assert lib.orbx_bundle_adjust_landmarks_pnp_device(None, 1.0, 10, None) == bad


def test_record_offsets_and_block_layouts(pkg, tmp_path):
    exe = tmp_path / "pnp_layout_pins.bin"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(rocm, "include"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "cpp", "pnp_layout_pins.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    m = re.search(r"(\d+) values compared, (\d+) failures", r.stdout)
    assert m and int(m.group(2)) == 0 and int(m.group(1)) == 256 * 6 * 5 * 8
    for line, struct in ((r.stdout.splitlines()[0], pkg.orbx_pnp.PnpRecord),
                         (r.stdout.splitlines()[1], pkg.orbx_pnp.WindowPosesPnpView)):
        words = line.split()
        assert int(words[2]) == C.sizeof(struct)
        got = dict(zip(words[3::2], map(int, words[4::2])))
        assert got == {f: getattr(struct, f).offset for f, _ in struct._fields_}, line
