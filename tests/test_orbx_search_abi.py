"""The ninth public header, include/orbx_search.h, against the binding's ninth prototype table
(orbx_search.PROTOTYPES), the way tests/test_orbx_prior_abi.py pins include/orbx_prior.h: every function declared with
the header's parameter classes, the views and the enum with the header's fields and values, the prototypes applied in
one place, every symbol exported by liborbx.so, every declaration citing the reference, the rules restated in header
and design, and the entries refusing a NULL context without a GPU.  The first eight headers and tables stay as they
were: nothing of rank 21 is in them."""
import ctypes as C
import inspect
import os
import re

import numpy as np

from test_binding_prototypes import RETURNS, SCALARS, is_pointer
from test_orbx_pnp_abi import struct_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("orbx_landmarks_project_device", "orbx_landmarks_project_results_device", "orbx_landmarks_project_fetch",
           "orbx_project_landmarks", "orbx_reassociate_gated_device", "orbx_reassociate_gated_results_device",
           "orbx_reassociate_gated_fetch", "orbx_reassociate_gated")
OTHER_HEADERS = ("orbx.h", "orbx_vo.h", "orbx_lm.h", "orbx_stream.h", "orbx_pnp.h", "orbx_carry.h", "orbx_reloc.h",
                 "orbx_prior.h")
CITES = ("src/with_bundle_adjustment.cpp:586-593", "src/feature_tracking.cpp:203-219")
RULES = ("P1", "P2", "P3", "P4", "P5", "K", "L", "M", "N")


def raw_header(name="orbx_search.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def header(name="orbx_search.h"):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", raw_header(name), flags=re.S))


def declarations(name="orbx_search.h"):
    src = header(name)
    out = {}
    for ret, fn, params in re.findall(r"^([A-Za-z_][\w \t\*]*?)\s*\b(orbx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        params = [" ".join(p.split()) for p in params.split(",")]
        out[fn] = (re.sub(r"\s*\*", "*", " ".join(ret.split())), [] if params == ["void"] else params)
    assert sorted(out) == sorted(set(re.findall(r"\b(orbx_[a-z0-9_]+)\s*\(", src)))  # no declaration slipped through
    return out


def names(fn, h="orbx_search.h"):
    return [p.replace("*", " ").split()[-1] for p in declarations(h)[fn][1]]


def test_table_against_header(pkg):
    table, decls = pkg.orbx_search.PROTOTYPES, declarations()
    assert sorted(decls) == sorted(table) == sorted(ENTRIES) and pkg.orbx_search.EXPORTS == list(table)
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
    assert names("orbx_landmarks_project_device") == ["ctx", "K", "d_pose6", "pose_stride", "n_windows", "source",
                                                      "width", "height", "margin_px", "stream"]
    assert names("orbx_landmarks_project_results_device") == ["ctx", "view"]
    assert names("orbx_landmarks_project_fetch") == ["ctx", "first", "n", "xy", "depth", "state", "count"]
    # the host entry takes an old window as orbx_localise_carried_window takes it
    old = names("orbx_localise_carried_window", "orbx_carry.h")[1:4]
    assert old == ["old_points3", "old_slot_of_point", "n_old"]
    assert names("orbx_project_landmarks") == ["ctx", "points3", "slot_of_point", "n_old", "slot_capacity", "K", "pose6",
                                               "width", "height", "margin_px", "xy", "depth", "state", "count"]
    gated = names("orbx_reassociate_gated_device")
    assert gated == ["ctx", "d_query_desc", "d_query_state", "d_query_xy", "point_stride", "xy_frame_stride",
                     "q_capacity", "d_train_desc", "d_train_state", "d_train_xy", "d_train_pstate", "t_capacity",
                     "n_windows", "radius_px", "ratio", "max_distance", "accept_lone", "unique", "stream"]
    # desc / state / capacities / ratio / max_distance / unique are exactly what orbx_reassociate_device takes, in its
    # order; the point source has the strides of orbx_describe_points_device
    base = names("orbx_reassociate_device", "orbx_reloc.h")
    extra = {"d_query_xy", "point_stride", "xy_frame_stride", "d_train_xy", "d_train_pstate", "radius_px", "accept_lone"}
    assert [p for p in gated if p not in extra] == base
    described = names("orbx_describe_points_device", "orbx_reloc.h")
    assert all(p in described for p in ("point_stride", "xy_frame_stride"))
    d, r = declarations(), declarations("orbx_reloc.h")
    for p in ("point_stride", "xy_frame_stride"):
        mine = d["orbx_reassociate_gated_device"][1][gated.index(p)]
        assert mine == r["orbx_describe_points_device"][1][described.index(p)] == "size_t " + p
    assert d["orbx_reassociate_gated_device"][1][gated.index("d_train_xy")] == "const double* d_train_xy"
    assert d["orbx_reassociate_gated_device"][1][gated.index("d_query_xy")] == "const float* d_query_xy"
    assert names("orbx_reassociate_gated_results_device") == ["ctx", "view"]
    assert names("orbx_reassociate_gated_fetch") == ["ctx", "first", "n", "candidates"]
    host = names("orbx_reassociate", "orbx_reloc.h")
    extra = {"query_xy", "train_xy", "train_pstate", "radius_px", "accept_lone", "candidates"}
    assert [p for p in names("orbx_reassociate_gated") if p not in extra] == host
    assert names("orbx_reassociate_gated")[-1] == "candidates"


def test_views_and_enum_against_header(pkg):
    o = pkg.orbx_search
    structs = dict((n, b) for b, n in re.findall(r"typedef\s+struct\s*\{([^}]*)\}\s*(orbx_\w+)\s*;", header()))
    assert sorted(structs) == ["orbx_landmarks_projection_view", "orbx_reassociate_gated_view"]
    for name, cls, fields, size in (
            ("orbx_landmarks_projection_view", o.LandmarksProjectionView,
             ["xy", "depth", "state", "count", "slot_capacity", "n_windows"], 4 * 8 + 2 * 4),
            ("orbx_reassociate_gated_view", o.ReassociateGatedView, ["candidates", "q_capacity", "n_windows"],
             8 + 2 * 4)):
        view = struct_fields(structs[name])
        assert [(f, is_pointer(t)) for f, t in cls._fields_] == [(f, p) for f, p, _, _ in view], name
        assert all(p or c == "int32_t" for _, p, c, _ in view)
        assert all(t is C.c_int32 for _, t in cls._fields_ if not is_pointer(t))
        assert [f for f, _ in cls._fields_] == fields and C.sizeof(cls) == size, name
    enums = dict((n, int(v)) for n, v in re.findall(r"\b(ORBX_PROJ_[A-Z_]+)\s*=\s*(\d+)", header()))
    assert enums == dict(ORBX_PROJ_NONE=o.PROJ_NONE, ORBX_PROJ_BEHIND=o.PROJ_BEHIND, ORBX_PROJ_OUTSIDE=o.PROJ_OUTSIDE,
                         ORBX_PROJ_OK=o.PROJ_OK)
    assert o.PROJ_NONE == 0 and (o.PROJ_BEHIND, o.PROJ_OUTSIDE, o.PROJ_OK) == (1, 2, 3)
    assert re.search(r"\}\s*orbx_proj_state\s*;", header())
    # the view's xy and state are what the gated entry takes as d_train_xy and d_train_pstate
    view = dict((f, c) for f, _, c, _ in struct_fields(structs["orbx_landmarks_projection_view"]))
    assert "double" in view["xy"] and "int32_t" in view["state"]


def test_no_symbol_of_the_other_eight_headers_is_declared_again(pkg):
    mine = set(declarations())
    others = [pkg.orbx, pkg.orbx_vo, pkg.orbx_lm, pkg.orbx_stream, pkg.orbx_pnp, pkg.orbx_carry, pkg.orbx_reloc,
              pkg.orbx_prior]
    for name, mod in zip(OTHER_HEADERS, others):
        theirs = set(declarations(name))
        assert not (mine & theirs), (name, mine & theirs)
        assert not (set(pkg.orbx_search.PROTOTYPES) & set(mod.PROTOTYPES)), name
        for entry in ENTRIES:
            assert not re.search(r"\b%s\b" % entry, raw_header(name)), (name, entry)
    assert len(declarations("orbx.h")) == 94  # the first header stays at its 94 declarations
    includes = re.findall(r'#include\s+"([^"]+)"', raw_header())
    assert includes == ["orbx.h", "orbx_carry.h"]  # the first and, for orbx_carry_source, the sixth
    assert pkg.orbx_search.load() is pkg.orbx.load()


def test_prototypes_are_set_in_load_and_nowhere_else(pkg):
    o = pkg.orbx_search
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
    assert "orbx_search.EXPORTS" in inspect.getsource(__graft_entry__.build)
    assert pkg.orbx_search is not None and "orbx_search" in open(
        os.path.join(ROOT, "visual-odometry-gpu_amd", "__init__.py")).read()


def test_the_declarations_cite_the_reference():
    src = raw_header()
    for name in ENTRIES:
        at = src.index("int %s(" % name)
        comment = src[:at].rsplit("/*", 1)[1]
        assert any(c in comment for c in CITES), name
    for view in ("orbx_landmarks_projection_view", "orbx_reassociate_gated_view"):
        at = src.index("} %s;" % view)
        comment = src[:at].rsplit("typedef struct", 1)[0].rsplit("/*", 1)[1]
        assert any(c in comment for c in CITES), view


def test_the_rules_are_restated_in_header_and_design():
    head = raw_header().split("#ifndef")[0]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "**Rank 21" in design
    rank21 = design.split("**Rank 21", 1)[1]
    for rule in RULES:
        assert re.search(r"^ \*   %s [a-z0-9]" % rule, head, flags=re.M), rule
        assert re.search(r"^%s [a-z0-9]" % rule, rank21, flags=re.M), rule
    for words in ("ba_pose_prepare", "BA_MAX_THETA", "pnp_inlier", "(d << 22) | t", "accept_lone", "radius_px * radius_px",
                  "margin_px"):
        assert words in head and words in rank21, words


def test_the_functions_take_a_context(pkg):
    for f in ("landmarks_project", "landmarks_project_view", "landmarks_project_fetch", "project_landmarks_host",
              "reassociate_gated", "reassociate_gated_view", "reassociate_gated_fetch", "reassociate_gated_host"):
        assert list(inspect.signature(getattr(pkg.orbx_search, f)).parameters)[0] == "ctx", f
    src = inspect.getsource(pkg.orbx_search)
    assert "_f64(" in src and "_stream(" in src and "_count(" in src and "_device_arg(" in src


def test_without_a_context_the_entries_refuse(pkg):
    """a NULL context is ORBX_ERR_INVALID_ARG before anything touches a device, as for every entry of the other
    headers"""
    lib = pkg.orbx_search.load()
    K = np.eye(3)
    bad = pkg.orbx.ERR_INVALID_ARG
    assert lib.orbx_landmarks_project_device(None, K.ctypes.data, None, 6, 1, 0, 10, 10, 0.0, None) == bad
    assert lib.orbx_landmarks_project_results_device(None, None) == bad
    assert lib.orbx_landmarks_project_fetch(None, 0, 1, None, None, None, None) == bad
    assert lib.orbx_project_landmarks(None, None, None, 0, 1, K.ctypes.data, None, 10, 10, 0.0, None, None, None,
                                      None) == bad
    assert lib.orbx_reassociate_gated_device(None, None, None, None, 2, 2, 1, None, None, None, None, 1, 1, 1.0, 0.8,
                                             256, 0, 1, None) == bad
    assert lib.orbx_reassociate_gated_results_device(None, None) == bad
    assert lib.orbx_reassociate_gated_fetch(None, 0, 1, None) == bad
    assert lib.orbx_reassociate_gated(None, None, None, None, 0, None, None, None, None, 0, 1.0, 0.8, 256, 0, 1, None,
                                      None, None, None) == bad
