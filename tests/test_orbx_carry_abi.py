"""CPU-only checks of the sixth public header, include/orbx_carry.h, against the binding's sixth prototype table
(orbx_carry.PROTOTYPES), the way tests/test_orbx_pnp_abi.py pins include/orbx_pnp.h: every function declared with the
header's parameter classes, the views and enums with the header's fields and values, the prototypes applied in one
place, every symbol exported by liborbx.so, every declaration citing the reference -- and, without a GPU, the entries
refusing as the others do.  The first five headers and tables stay as they were: nothing of rank 18 is in them."""
import ctypes as C
import inspect
import os
import re

import numpy as np

from test_binding_prototypes import RETURNS, SCALARS, is_pointer
from test_orbx_pnp_abi import struct_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("orbx_landmarks_carry_device", "orbx_landmarks_carry_results_device", "orbx_landmarks_carry_fetch",
           "orbx_window_poses_pnp_carried_device", "orbx_window_poses_pnp_carried_results_device",
           "orbx_window_poses_pnp_carried_fetch", "orbx_window_poses_pnp_carried_mask_fetch",
           "orbx_landmarks_build_carried_device", "orbx_localise_carried_window")
OTHER_HEADERS = ("orbx.h", "orbx_vo.h", "orbx_lm.h", "orbx_stream.h", "orbx_pnp.h")
CITES = ("src/with_bundle_adjustment.cpp:586-593", "src/with_bundle_adjustment.cpp:196-208")
PNP_ARGS = ["prob", "threshold_px", "max_iters", "seed", "refine_iters", "min_inliers"]


def raw_header(name="orbx_carry.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def header(name="orbx_carry.h"):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", raw_header(name), flags=re.S))


def declarations(name="orbx_carry.h"):
    src = header(name)
    out = {}
    for ret, fn, params in re.findall(r"^([A-Za-z_][\w \t\*]*?)\s*\b(orbx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        params = [" ".join(p.split()) for p in params.split(",")]
        out[fn] = (re.sub(r"\s*\*", "*", " ".join(ret.split())), [] if params == ["void"] else params)
    assert sorted(out) == sorted(set(re.findall(r"\b(orbx_[a-z0-9_]+)\s*\(", src)))  # no declaration slipped through
    return out


def test_table_against_header(pkg):
    table, decls = pkg.orbx_carry.PROTOTYPES, declarations()
    assert sorted(decls) == sorted(table) == sorted(ENTRIES) and pkg.orbx_carry.EXPORTS == list(table)
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


def test_the_signatures_are_the_issued_ones(pkg):
    d = declarations()
    names = lambda fn: [p.replace("*", " ").split()[-1] for p in d[fn][1]]
    assert names("orbx_landmarks_carry_device") == ["ctx", "d_origin", "n_windows", "slot_capacity", "source", "stream"]
    assert names("orbx_landmarks_carry_fetch") == ["ctx", "first", "n", "xyz", "point", "count"]
    sizes = ["n_windows", "slot_capacity", "window_len"]
    assert names("orbx_window_poses_pnp_carried_device") == ["ctx", "K", "d_tracks_xy", "d_seen"] + sizes + PNP_ARGS + \
        ["stream"]
    assert names("orbx_window_poses_pnp_carried_fetch") == ["ctx", "first", "n", "records", "poses6", "window_status"]
    assert names("orbx_window_poses_pnp_carried_mask_fetch") == ["ctx", "window", "k", "mask", "capacity", "count"]
    assert names("orbx_landmarks_build_carried_device") == ["ctx", "K", "d_tracks_xy", "d_seen"] + sizes + ["stream"]
    assert names("orbx_localise_carried_window") == \
        ["ctx", "old_points3", "old_slot_of_point", "n_old", "origin", "tracks_xy", "seen", "n_slots", "window_len",
         "K"] + PNP_ARGS + ["records", "poses6", "window_status", "carried_point"]
    # the PnP parameters have the classes orbx_pnp_ransac gives them; the carried build is the chained build's shape
    pnp = pkg.orbx_pnp.PROTOTYPES["orbx_pnp_ransac"][1][5:11]
    assert pkg.orbx_carry.PROTOTYPES["orbx_window_poses_pnp_carried_device"][1][7:13] == pnp
    assert pkg.orbx_carry.PROTOTYPES["orbx_localise_carried_window"][1][10:16] == pnp
    assert pkg.orbx_carry.PROTOTYPES["orbx_landmarks_build_carried_device"] == \
        pkg.orbx_vo.PROTOTYPES["orbx_landmarks_build_chained_device"]


def test_views_and_enums_against_header(pkg):
    o = pkg.orbx_carry
    structs = dict((n, b) for b, n in re.findall(r"typedef\s+struct\s*\{([^}]*)\}\s*(orbx_\w+)\s*;", header()))
    assert sorted(structs) == ["orbx_landmarks_carry_view", "orbx_window_poses_carried_view"]
    for name, cls, size in (("orbx_landmarks_carry_view", o.LandmarksCarryView, 3 * 8 + 2 * 4),
                            ("orbx_window_poses_carried_view", o.WindowPosesCarriedView, 4 * 8 + 3 * 4 + 4)):
        view = struct_fields(structs[name])
        assert [(f, is_pointer(t)) for f, t in cls._fields_] == [(f, p) for f, p, _, _ in view], name
        assert all(p or c == "int32_t" for _, p, c, _ in view)
        assert all(t is C.c_int32 for _, t in cls._fields_ if not is_pointer(t))
        assert C.sizeof(cls) == size, name
    assert [f for f, _ in o.LandmarksCarryView._fields_] == ["xyz", "point", "count", "slot_capacity", "n_windows"]
    assert [f for f, _ in o.WindowPosesCarriedView._fields_] == ["records", "poses6", "mask", "window_status",
                                                                  "slot_capacity", "window_len", "n_windows"]
    enums = dict((n, int(v)) for n, v in re.findall(r"\b(ORBX_CARRY_[A-Z_]+)\s*=\s*(\d+)", header()))
    assert enums == dict(ORBX_CARRY_BUILT=o.CARRY_BUILT, ORBX_CARRY_SOLVED=o.CARRY_SOLVED, ORBX_CARRY_OK=o.CARRY_OK,
                         ORBX_CARRY_LOST=o.CARRY_LOST)
    assert (o.CARRY_BUILT, o.CARRY_SOLVED, o.CARRY_OK, o.CARRY_LOST) == (0, 1, 0, 1)
    # ORBX_CARRY_OK is 0: the build reads window_status as it reads the chain's status, and 0 is the good one there
    assert re.search(r"ORBX_WP_OK\s*=\s*0", header("orbx_vo.h"))
    assert o.RECORD_DTYPE is pkg.orbx_pnp.RECORD_DTYPE  # the record is rank 17's


def test_no_symbol_of_the_other_five_headers_is_declared_again(pkg):
    mine = set(declarations())
    others = [pkg.orbx, pkg.orbx_vo, pkg.orbx_lm, pkg.orbx_stream, pkg.orbx_pnp]
    for name, mod in zip(OTHER_HEADERS, others):
        theirs = set(declarations(name))
        assert not (mine & theirs), (name, mine & theirs)
        assert not (set(pkg.orbx_carry.PROTOTYPES) & set(mod.PROTOTYPES)), name
        for entry in ENTRIES:
            assert entry not in raw_header(name), (name, entry)
    assert len(declarations("orbx.h")) == 94  # the first header stays at its 94 declarations
    includes = re.findall(r'#include\s+"([^"]+)"', raw_header())
    assert includes == ["orbx.h", "orbx_pnp.h"]  # the sixth header includes the first and, for the record, the fifth
    assert pkg.orbx_carry.load() is pkg.orbx.load()


def test_prototypes_are_set_in_load_and_nowhere_else(pkg):
    o = pkg.orbx_carry
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
    assert "orbx_carry.EXPORTS" in inspect.getsource(__graft_entry__.build)


def test_the_declarations_cite_the_reference():
    src = raw_header()
    for name in ENTRIES:
        at = src.index("int %s(" % name)
        comment = src[:at].rsplit("/*", 1)[1]
        assert any(c in comment for c in CITES), name
    for struct in ("orbx_landmarks_carry_view", "orbx_window_poses_carried_view"):
        at = src.index("} %s;" % struct)
        comment = src[:at].rsplit("typedef struct", 1)[0].rsplit("/*", 1)[1]
        assert any(c in comment for c in CITES), struct


def test_the_functions_take_a_context(pkg):
    for f in ("landmarks_carry", "landmarks_carry_view", "landmarks_carry_fetch", "window_poses_pnp_carried",
              "window_poses_pnp_carried_view", "window_poses_pnp_carried_fetch", "window_poses_pnp_carried_mask",
              "landmarks_build_carried", "localise_carried_window"):
        assert list(inspect.signature(getattr(pkg.orbx_carry, f)).parameters)[0] == "ctx", f
    src = inspect.getsource(pkg.orbx_carry)
    assert "_f64(" in src and "_stream(" in src and "_count(" in src  # arguments through orbx's helpers
    assert "_tracks_args(" in src and "_device_arg(" in src


def test_without_a_context_the_entries_refuse(pkg):
    """a NULL context is ORBX_ERR_INVALID_ARG before anything touches a device, as for every entry of the other
    headers"""
    lib = pkg.orbx_carry.load()
    K = np.eye(3)
    bad = pkg.orbx.ERR_INVALID_ARG
    assert lib.orbx_landmarks_carry_device(None, None, 1, 1, 0, None) == bad
    assert lib.orbx_landmarks_carry_results_device(None, None) == bad
    assert lib.orbx_landmarks_carry_fetch(None, 0, 1, None, None, None) == bad
    assert lib.orbx_window_poses_pnp_carried_device(None, K.ctypes.data, None, None, 1, 1, 4, 0.99, 2.0, 10, 0, 10, 4,
                                                    None) == bad
    assert lib.orbx_window_poses_pnp_carried_results_device(None, None) == bad
    assert lib.orbx_window_poses_pnp_carried_fetch(None, 0, 1, None, None, None) == bad
    assert lib.orbx_window_poses_pnp_carried_mask_fetch(None, 0, 0, None, 0, None) == bad
    assert lib.orbx_landmarks_build_carried_device(None, K.ctypes.data, None, None, 1, 1, 4, None) == bad
    assert lib.orbx_localise_carried_window(None, None, None, 0, None, None, None, 1, 4, K.ctypes.data, 0.99, 2.0, 10,
                                            0, 10, 4, None, None, None, None) == bad
