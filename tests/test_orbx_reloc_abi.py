"""The seventh public header, include/orbx_reloc.h, against the binding's seventh prototype table
(orbx_reloc.PROTOTYPES), the way tests/test_orbx_carry_abi.py pins include/orbx_carry.h: every function declared with
the header's parameter classes, the views and the enum with the header's fields and values, the prototypes applied in
one place, every symbol exported by liborbx.so, every declaration citing the reference, the entries refusing a NULL
context without a GPU -- and, on the GPU, every argument error launching and writing nothing while the previous
results stay fetchable.  The first six headers and tables stay as they were: nothing of rank 19 is in them."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from test_binding_prototypes import RETURNS, SCALARS, is_pointer
from test_orbx_pnp_abi import struct_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("orbx_describe_points_device", "orbx_describe_points_workspace_limit",
           "orbx_point_descriptors_results_device", "orbx_point_descriptors_fetch", "orbx_describe_points",
           "orbx_reassociate_device", "orbx_reassociate_results_device", "orbx_reassociate_fetch", "orbx_reassociate")
OTHER_HEADERS = ("orbx.h", "orbx_vo.h", "orbx_lm.h", "orbx_stream.h", "orbx_pnp.h", "orbx_carry.h")
CITES = ("src/feature_tracking.cpp:68-71", "src/feature_tracking.cpp:203-219")


def raw_header(name="orbx_reloc.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def header(name="orbx_reloc.h"):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", raw_header(name), flags=re.S))


def declarations(name="orbx_reloc.h"):
    src = header(name)
    out = {}
    for ret, fn, params in re.findall(r"^([A-Za-z_][\w \t\*]*?)\s*\b(orbx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        params = [" ".join(p.split()) for p in params.split(",")]
        out[fn] = (re.sub(r"\s*\*", "*", " ".join(ret.split())), [] if params == ["void"] else params)
    assert sorted(out) == sorted(set(re.findall(r"\b(orbx_[a-z0-9_]+)\s*\(", src)))  # no declaration slipped through
    return out


def test_table_against_header(pkg):
    table, decls = pkg.orbx_reloc.PROTOTYPES, declarations()
    assert sorted(decls) == sorted(table) == sorted(ENTRIES) and pkg.orbx_reloc.EXPORTS == list(table)
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
    frames = ["d_frames", "n", "width", "height", "row_stride", "frame_stride"]
    assert names("orbx_describe_points_device") == ["ctx"] + frames + \
        ["d_xy", "point_stride", "xy_frame_stride", "d_seen", "seen_min", "d_counts", "slot_capacity", "bank", "stream"]
    # the frames as orbx_good_features_batch_device takes them, the point source as the top-up takes its seeds
    gf = pkg.orbx.PROTOTYPES["orbx_good_features_batch_device"][1]
    topup = pkg.orbx.PROTOTYPES["orbx_good_features_topup_device"][1]
    mine = pkg.orbx_reloc.PROTOTYPES["orbx_describe_points_device"][1]
    assert mine[:7] == gf[:7] == topup[:7] and mine[7:12] == topup[7:12]
    assert names("orbx_point_descriptors_results_device") == ["ctx", "bank", "view"]
    assert names("orbx_point_descriptors_fetch") == ["ctx", "bank", "first", "n", "desc", "angle", "state", "n_ok"]
    assert names("orbx_describe_points") == ["ctx", "image", "width", "height", "stride", "points_xy", "n_points",
                                             "angle", "desc", "state"]
    assert names("orbx_reassociate_device") == ["ctx", "d_query_desc", "d_query_state", "q_capacity", "d_train_desc",
                                                "d_train_state", "t_capacity", "n_windows", "ratio", "max_distance",
                                                "unique", "stream"]
    assert names("orbx_reassociate_fetch") == ["ctx", "first", "n", "origin", "dist", "count"]
    assert names("orbx_reassociate") == ["ctx", "query_desc", "query_state", "nq", "train_desc", "train_state", "nt",
                                         "ratio", "max_distance", "unique", "origin", "dist", "count"]


def test_views_and_enums_against_header(pkg):
    o = pkg.orbx_reloc
    structs = dict((n, b) for b, n in re.findall(r"typedef\s+struct\s*\{([^}]*)\}\s*(orbx_\w+)\s*;", header()))
    assert sorted(structs) == ["orbx_point_descriptors_view", "orbx_reassociate_view"]
    for name, cls, size in (("orbx_point_descriptors_view", o.PointDescriptorsView, 4 * 8 + 2 * 4),
                            ("orbx_reassociate_view", o.ReassociateView, 3 * 8 + 3 * 4 + 4)):
        view = struct_fields(structs[name])
        assert [(f, is_pointer(t)) for f, t in cls._fields_] == [(f, p) for f, p, _, _ in view], name
        assert all(p or c == "int32_t" for _, p, c, _ in view)
        assert all(t is C.c_int32 for _, t in cls._fields_ if not is_pointer(t))
        assert C.sizeof(cls) == size, name
    assert [f for f, _ in o.PointDescriptorsView._fields_] == ["desc", "angle", "state", "n_ok", "slot_capacity", "n"]
    assert [f for f, _ in o.ReassociateView._fields_] == ["origin", "dist", "count", "q_capacity", "t_capacity",
                                                           "n_windows"]
    enums = dict((n, int(v)) for n, v in re.findall(r"\b(ORBX_PD_[A-Z]+)\s*=\s*(\d+)", header()))
    assert enums == dict(ORBX_PD_NONE=o.PD_NONE, ORBX_PD_BORDER=o.PD_BORDER, ORBX_PD_OK=o.PD_OK)
    assert (o.PD_NONE, o.PD_BORDER, o.PD_OK) == (0, 1, 2)  # NONE is 0: a zeroed state array describes nothing
    assert re.search(r"#define\s+ORBX_PD_BANKS\s+2\b", header()) and o.PD_BANKS == 2
    m = re.search(r"#define\s+ORBX_PD_WORKSPACE_DEFAULT\s+\(\(size_t\)(\d+)\s*<<\s*(\d+)\)", header())
    assert m and int(m.group(1)) << int(m.group(2)) == o.PD_WORKSPACE_DEFAULT
    # view.origin is what the carry takes: int32 [n_windows][slot_capacity]
    carry = re.sub(r"\s+", " ", header("orbx_carry.h"))
    assert "int orbx_landmarks_carry_device(orbx_ctx* ctx, const int32_t* d_origin, int n_windows, int slot_capacity" in carry
    assert re.search(r"const int32_t\*\s*origin;", header())


def test_no_symbol_of_the_other_six_headers_is_declared_again(pkg):
    mine = set(declarations())
    others = [pkg.orbx, pkg.orbx_vo, pkg.orbx_lm, pkg.orbx_stream, pkg.orbx_pnp, pkg.orbx_carry]
    for name, mod in zip(OTHER_HEADERS, others):
        theirs = set(declarations(name))
        assert not (mine & theirs), (name, mine & theirs)
        assert not (set(pkg.orbx_reloc.PROTOTYPES) & set(mod.PROTOTYPES)), name
        for entry in ENTRIES:
            assert entry not in raw_header(name), (name, entry)
    assert len(declarations("orbx.h")) == 94  # the first header stays at its 94 declarations
    assert re.findall(r'#include\s+"([^"]+)"', raw_header()) == ["orbx.h"]
    assert pkg.orbx_reloc.load() is pkg.orbx.load()


def test_prototypes_are_set_in_load_and_nowhere_else(pkg):
    o = pkg.orbx_reloc
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
    assert "orbx_reloc.EXPORTS" in inspect.getsource(__graft_entry__.build)


def test_the_declarations_cite_the_reference():
    src = raw_header()
    for name in ENTRIES:
        at = src.index("int %s(" % name)
        comment = src[:at].rsplit("/*", 1)[1]
        assert any(c in comment for c in CITES), name
    for struct in ("orbx_point_descriptors_view", "orbx_reassociate_view"):
        at = src.index("} %s;" % struct)
        comment = src[:at].rsplit("typedef struct", 1)[0].rsplit("/*", 1)[1]
        assert any(c in comment for c in CITES), struct


def test_the_rules_are_restated(pkg):
    """rules A-J stand in the header and in DESIGN.md §9 rank 19, with rule C's R"""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "**Rank 19" in design
    for text in (raw_header(), design[design.index("**Rank 19"):]):
        for rule in ("A live", "B pixel", "C interior", "D image", "E values", "F sets", "G 2-NN", "H accept",
                     "I unique", "J out"):
            assert rule in text, rule
        assert "max(patch_size / 2, 20)" in text and "18.38" in text


def test_the_functions_take_a_context(pkg):
    for f in ("describe_points", "describe_points_workspace_limit", "point_descriptors_view",
              "point_descriptors_fetch", "describe_points_host", "reassociate", "reassociate_view",
              "reassociate_fetch", "reassociate_host"):
        assert list(inspect.signature(getattr(pkg.orbx_reloc, f)).parameters)[0] == "ctx", f
    src = inspect.getsource(pkg.orbx_reloc)
    assert "_frames_arg(" in src and "_stream(" in src and "_count(" in src and "_device_arg(" in src


def test_without_a_context_the_entries_refuse(pkg):
    """a NULL context is ORBX_ERR_INVALID_ARG before anything touches a device"""
    lib = pkg.orbx_reloc.load()
    bad = pkg.orbx.ERR_INVALID_ARG
    assert lib.orbx_describe_points_device(None, None, 1, 8, 8, 8, 64, None, 2, 2, None, 0, None, 1, 0, None) == bad
    assert lib.orbx_describe_points_workspace_limit(None, 0) == bad
    assert lib.orbx_point_descriptors_results_device(None, 0, None) == bad
    assert lib.orbx_point_descriptors_fetch(None, 0, 0, 1, None, None, None, None) == bad
    assert lib.orbx_describe_points(None, None, 8, 8, 8, None, 0, None, None, None) == bad
    assert lib.orbx_reassociate_device(None, None, None, 1, None, None, 1, 1, 0.8, 256, 1, None) == bad
    assert lib.orbx_reassociate_results_device(None, None) == bad
    assert lib.orbx_reassociate_fetch(None, 0, 1, None, None, None) == bad
    assert lib.orbx_reassociate(None, None, None, 0, None, None, 0, 0.8, 256, 1, None, None, None) == bad


def test_the_point_source_helper_refuses(pkg):
    """the binding's own refusals, without a GPU"""
    import torch

    from test_binding_prototypes import on_device, refused

    o = pkg.orbx_reloc
    assert refused(o._points_arg, 0x1000, 2, None, 2, 10, []) == \
        "a raw points address needs slot_capacity, point_stride and frame_stride"
    assert o._points_arg(0x1000, 2, 5, 10, 50, []) == (0x1000, 5, 10, 50, False)
    msg = "points must be (n, slots, 2) float32 on the device with unit stride along the pair"
    tracks = on_device(torch.zeros((2, 5, 4, 2)))
    assert refused(o._points_arg, torch.zeros((2, 5, 2)), 2, None, None, None, []) == msg  # a CPU tensor
    assert refused(o._points_arg, tracks[:, :, 1], 3, None, None, None, []) == msg          # another n
    assert refused(o._points_arg, tracks[:, :, :2, 0], 2, None, None, None, []) == msg      # pair stride 2
    view = tracks[:, :, 3]  # frame 3 of an LK tracks block: point_stride 2 * window_len
    assert o._points_arg(view, 2, None, None, None, []) == (tracks.data_ptr() + 4 * 6, 5, 8, 40, False)
    assert refused(o._points_arg, view, 2, 6, None, None, []) == "slot_capacity differs from points.shape[1]"
    assert refused(o._set_arg, 0x1000, 0x2000, None, None, "query", []) == \
        "a raw query address needs n_windows and its capacity"
    v = o.PointDescriptorsView(desc=0x1000, angle=0x2000, state=0x3000, n_ok=0x4000, slot_capacity=9, n=4)
    assert o._set_arg(v, None, None, None, "train", []) == (0x1000, 0x3000, 4, 9, False)


# ---- argument errors, on the GPU ------------------------------------------------------------------------------------
def _ptrs(*tensors):
    return [t.data_ptr() for t in tensors]


@pytest.mark.gpu
def test_argument_errors_launch_and_write_nothing(pkg):
    import torch

    import reassoc_ref as R

    o, bad, unsup = pkg.orbx_reloc, pkg.orbx.ERR_INVALID_ARG, pkg.orbx.ERR_UNSUPPORTED
    lib = o.load()
    rng = np.random.default_rng(3)
    frames = torch.from_numpy(rng.integers(0, 256, (2, 64, 96), dtype=np.uint8)).cuda()
    pts = torch.from_numpy(np.stack([rng.uniform(0, 95, (2, 12)), rng.uniform(0, 63, (2, 12))], -1).astype(np.float32)).cuda()
    seen = torch.ones((2, 12), dtype=torch.int32).cuda()
    counts = torch.full((2,), 12, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    with pkg.Context(pkg.default_params("gpu", max_width=96, max_height=64, max_batch=2)) as ctx:
        h = ctx._h
        F, X, S, N = _ptrs(frames, pts, seen, counts)
        good = [h, F, 2, 96, 64, 96, 96 * 64, X, 2, 24, S, 1, N, 12, 0, None]

        def describe(**change):
            names = ["ctx", "d_frames", "n", "width", "height", "row_stride", "frame_stride", "d_xy", "point_stride",
                     "xy_frame_stride", "d_seen", "seen_min", "d_counts", "slot_capacity", "bank", "stream"]
            args = list(good)
            for k, v in change.items():
                args[names.index(k)] = v
            return lib.orbx_describe_points_device(*args)

        # before anything has run: nothing to view or fetch
        v, rv = o.PointDescriptorsView(), o.ReassociateView()
        assert lib.orbx_point_descriptors_results_device(h, 0, C.byref(v)) == bad
        assert lib.orbx_point_descriptors_fetch(h, 1, 0, 1, None, None, None, None) == bad
        assert lib.orbx_reassociate_results_device(h, C.byref(rv)) == bad
        assert lib.orbx_reassociate_fetch(h, 0, 1, None, None, None) == bad
        assert describe() == pkg.orbx.OK and describe(bank=1) == pkg.orbx.OK
        before = [o.point_descriptors_fetch(ctx, b) for b in (0, 1)]
        assert before[0]["n_ok"].sum() > 0
        for change in (dict(d_frames=None), dict(d_xy=None), dict(bank=-1), dict(bank=2), dict(slot_capacity=0),
                       dict(slot_capacity=-3), dict(n=0), dict(n=3), dict(width=4), dict(width=97), dict(row_stride=95),
                       dict(frame_stride=96 * 63 + 95), dict(point_stride=1), dict(xy_frame_stride=23),
                       dict(point_stride=3, xy_frame_stride=3 * 11 + 1), dict(d_xy=X + 2), dict(d_seen=S + 1),
                       dict(d_counts=N + 2)):
            assert describe(**change) == bad, change
            assert ctx._lib.orbx_last_error_string(h)
        assert lib.orbx_point_descriptors_results_device(h, 2, C.byref(v)) == bad
        assert lib.orbx_point_descriptors_results_device(h, 0, None) == bad
        assert lib.orbx_point_descriptors_fetch(h, 0, 1, 2, None, None, None, None) == bad  # [1, 3) of 2 frames
        assert lib.orbx_point_descriptors_fetch(h, 0, 0, 0, None, None, None, None) == bad
        img = np.zeros((64, 96), np.uint8)
        xy = np.zeros((3, 2), np.float32)
        assert lib.orbx_describe_points(h, None, 96, 64, 96, xy.ctypes.data, 3, None, None, None) == bad
        assert lib.orbx_describe_points(h, img.ctypes.data, 96, 64, 95, xy.ctypes.data, 3, None, None, None) == bad
        assert lib.orbx_describe_points(h, img.ctypes.data, 96, 64, 96, None, 3, None, None, None) == bad
        assert lib.orbx_describe_points(h, img.ctypes.data, 96, 64, 96, xy.ctypes.data, -1, None, None, None) == bad
        # the re-association
        qd, qs, td, ts = (torch.from_numpy(a).cuda() for a in R.synthetic_windows())
        torch.cuda.synchronize()
        QD, QS, TD, TS = _ptrs(qd, qs, td, ts)
        rgood = [h, QD, QS, 70, TD, TS, 300, 3, 0.8, 256, 1, None]

        def reassoc(**change):
            names = ["ctx", "qd", "qs", "q_capacity", "td", "ts", "t_capacity", "n_windows", "ratio", "max_distance",
                     "unique", "stream"]
            args = list(rgood)
            for k, v in change.items():
                args[names.index(k)] = v
            return lib.orbx_reassociate_device(*args)

        assert reassoc() == pkg.orbx.OK
        rbefore = o.reassociate_fetch(ctx)
        assert rbefore["count"][0] > 0
        for change in (dict(qd=None), dict(qs=None), dict(td=None), dict(ts=None), dict(q_capacity=0),
                       dict(t_capacity=0), dict(t_capacity=-1), dict(n_windows=0), dict(max_distance=-1),
                       dict(max_distance=257), dict(unique=2), dict(unique=-1), dict(ratio=float("nan")),
                       dict(ratio=float("inf")), dict(ratio=-0.5), dict(qd=QD + 8), dict(ts=TS + 2)):
            assert reassoc(**change) == bad, change
        assert reassoc(n_windows=65536) == unsup and reassoc(q_capacity=(1 << 22) + 1) == unsup
        assert lib.orbx_reassociate_fetch(h, 2, 2, None, None, None) == bad
        assert lib.orbx_reassociate_results_device(h, None) == bad
        d0, s0 = np.zeros((2, 32), np.uint8), np.full(2, R.PD_OK, np.int32)
        for args in ((None, s0.ctypes.data, 2, d0.ctypes.data, s0.ctypes.data, 2, 0.8, 256, 1),
                     (d0.ctypes.data, s0.ctypes.data, -1, d0.ctypes.data, s0.ctypes.data, 2, 0.8, 256, 1),
                     (d0.ctypes.data, s0.ctypes.data, 2, d0.ctypes.data, None, 2, 0.8, 256, 1),
                     (d0.ctypes.data, s0.ctypes.data, 2, d0.ctypes.data, s0.ctypes.data, 2, 0.8, 300, 1),
                     (d0.ctypes.data, s0.ctypes.data, 2, d0.ctypes.data, s0.ctypes.data, 2, 0.8, 256, 3)):
            assert lib.orbx_reassociate(h, *args, None, None, None) == bad, args
        # every previous result is still there, with the same bytes, and the context is usable
        for b in (0, 1):
            after = o.point_descriptors_fetch(ctx, b)
            for k in before[b]:
                assert after[k].tobytes() == before[b][k].tobytes(), (b, k)
        rafter = o.reassociate_fetch(ctx)
        for k in rbefore:
            assert rafter[k].tobytes() == rbefore[k].tobytes(), k
        assert describe() == pkg.orbx.OK and reassoc() == pkg.orbx.OK
