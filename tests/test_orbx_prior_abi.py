"""The eighth public header, include/orbx_prior.h, against the binding's eighth prototype table
(orbx_prior.PROTOTYPES), the way tests/test_orbx_carry_abi.py pins include/orbx_carry.h: every function declared with
the header's parameter classes, the view and the enum with the header's fields and values, the prototypes applied in
one place, every symbol exported by liborbx.so, every declaration citing the reference, and the entries refusing a
NULL context without a GPU.  The first seven headers and tables stay as they were: nothing of rank 20 is in them."""
import ctypes as C
import inspect
import os
import re

import numpy as np

from test_binding_prototypes import RETURNS, SCALARS, is_pointer
from test_orbx_pnp_abi import struct_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("orbx_bundle_adjust_prior", "orbx_bundle_adjust_prior_batch", "orbx_landmarks_priors_carried_device",
           "orbx_landmarks_priors_results_device", "orbx_landmarks_priors_fetch",
           "orbx_bundle_adjust_landmarks_prior_device")
OTHER_HEADERS = ("orbx.h", "orbx_vo.h", "orbx_lm.h", "orbx_stream.h", "orbx_pnp.h", "orbx_carry.h", "orbx_reloc.h")
CITES = ("src/with_bundle_adjustment.cpp:612-679", "src/with_bundle_adjustment.cpp:586-593")
PRIOR_ARGS = ["prior_xyz", "prior_weight", "start"]


def raw_header(name="orbx_prior.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def header(name="orbx_prior.h"):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", raw_header(name), flags=re.S))


def declarations(name="orbx_prior.h"):
    src = header(name)
    out = {}
    for ret, fn, params in re.findall(r"^([A-Za-z_][\w \t\*]*?)\s*\b(orbx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        params = [" ".join(p.split()) for p in params.split(",")]
        out[fn] = (re.sub(r"\s*\*", "*", " ".join(ret.split())), [] if params == ["void"] else params)
    assert sorted(out) == sorted(set(re.findall(r"\b(orbx_[a-z0-9_]+)\s*\(", src)))  # no declaration slipped through
    return out


def test_table_against_header(pkg):
    table, decls = pkg.orbx_prior.PROTOTYPES, declarations()
    assert sorted(decls) == sorted(table) == sorted(ENTRIES) and pkg.orbx_prior.EXPORTS == list(table)
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
    names = lambda fn, h="orbx_prior.h": [p.replace("*", " ").split()[-1] for p in (d if h == "orbx_prior.h" else
                                                                                     declarations(h))[fn][1]]
    # the two host entries are orbx_bundle_adjust / _batch with the three prior arguments in front of huber_delta
    for mine, theirs in (("orbx_bundle_adjust_prior", "orbx_bundle_adjust"),
                         ("orbx_bundle_adjust_prior_batch", "orbx_bundle_adjust_batch")):
        base = names(theirs, "orbx.h")
        at = base.index("huber_delta")
        assert names(mine) == base[:at] + PRIOR_ARGS + base[at:], mine
        bt, mt = pkg.orbx.PROTOTYPES[theirs], pkg.orbx_prior.PROTOTYPES[mine]
        assert mt[0] is bt[0] and mt[1][:at] == bt[1][:at] and mt[1][at + 3:] == bt[1][at:]
        assert is_pointer(mt[1][at]) and is_pointer(mt[1][at + 1]) and mt[1][at + 2] is C.c_int
    assert names("orbx_landmarks_priors_carried_device") == ["ctx", "weight", "stream"]
    assert names("orbx_landmarks_priors_results_device") == ["ctx", "view"]
    assert names("orbx_landmarks_priors_fetch") == ["ctx", "first", "n", "prior_xyz", "prior_weight", "count",
                                                    "capacity", "n_points"]
    # the device solve is orbx_bundle_adjust_landmarks_device with `start` in front of the stream
    base = names("orbx_bundle_adjust_landmarks_device", "orbx.h")
    assert names("orbx_bundle_adjust_landmarks_prior_device") == base[:-1] + ["start", "stream"]


def test_view_and_enum_against_header(pkg):
    o = pkg.orbx_prior
    structs = dict((n, b) for b, n in re.findall(r"typedef\s+struct\s*\{([^}]*)\}\s*(orbx_\w+)\s*;", header()))
    assert sorted(structs) == ["orbx_landmarks_priors_view"]
    view = struct_fields(structs["orbx_landmarks_priors_view"])
    cls = o.LandmarksPriorsView
    assert [(f, is_pointer(t)) for f, t in cls._fields_] == [(f, p) for f, p, _, _ in view]
    assert all(p or c == "int32_t" for _, p, c, _ in view)
    assert all(t is C.c_int32 for _, t in cls._fields_ if not is_pointer(t))
    assert [f for f, _ in cls._fields_] == ["prior", "count", "n_windows"]
    assert C.sizeof(cls) == 2 * 8 + 4 + 4  # (the int32 and the struct's tail padding)
    enums = dict((n, int(v)) for n, v in re.findall(r"\b(ORBX_PRIOR_[A-Z_]+)\s*=\s*(\d+)", header()))
    assert enums == dict(ORBX_PRIOR_START_GIVEN=o.PRIOR_START_GIVEN, ORBX_PRIOR_START_ANCHOR=o.PRIOR_START_ANCHOR)
    assert (o.PRIOR_START_GIVEN, o.PRIOR_START_ANCHOR) == (0, 1)
    assert re.search(r"\}\s*orbx_prior_start\s*;", header())


def test_no_symbol_of_the_other_seven_headers_is_declared_again(pkg):
    mine = set(declarations())
    others = [pkg.orbx, pkg.orbx_vo, pkg.orbx_lm, pkg.orbx_stream, pkg.orbx_pnp, pkg.orbx_carry, pkg.orbx_reloc]
    for name, mod in zip(OTHER_HEADERS, others):
        theirs = set(declarations(name))
        assert not (mine & theirs), (name, mine & theirs)
        assert not (set(pkg.orbx_prior.PROTOTYPES) & set(mod.PROTOTYPES)), name
        for entry in ENTRIES:
            assert not re.search(r"\b%s\b" % entry, raw_header(name)), (name, entry)
    assert len(declarations("orbx.h")) == 94  # the first header stays at its 94 declarations
    includes = re.findall(r'#include\s+"([^"]+)"', raw_header())
    assert includes == ["orbx.h", "orbx_carry.h"]  # the eighth header includes the first and, for rule P6, the sixth
    assert pkg.orbx_prior.load() is pkg.orbx.load()


def test_prototypes_are_set_in_load_and_nowhere_else(pkg):
    o = pkg.orbx_prior
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
    assert "orbx_prior.EXPORTS" in inspect.getsource(__graft_entry__.build)


def test_the_declarations_cite_the_reference():
    src = raw_header()
    for name in ENTRIES:
        at = src.index("int %s(" % name)
        comment = src[:at].rsplit("/*", 1)[1]
        assert any(c in comment for c in CITES), name
    at = src.index("} orbx_landmarks_priors_view;")
    comment = src[:at].rsplit("typedef struct", 1)[0].rsplit("/*", 1)[1]
    assert any(c in comment for c in CITES)


def test_the_functions_take_a_context(pkg):
    for f in ("bundle_adjust_prior", "bundle_adjust_prior_batch", "landmarks_priors_carried", "landmarks_priors_view",
              "landmarks_priors_fetch", "bundle_adjust_landmarks_prior"):
        assert list(inspect.signature(getattr(pkg.orbx_prior, f)).parameters)[0] == "ctx", f
    src = inspect.getsource(pkg.orbx_prior)
    assert "_f64(" in src and "_stream(" in src and "_count(" in src and "_observations(" in src


def test_without_a_context_the_entries_refuse(pkg):
    """a NULL context is ORBX_ERR_INVALID_ARG before anything touches a device, as for every entry of the other
    headers"""
    lib = pkg.orbx_prior.load()
    K = np.eye(3)
    bad = pkg.orbx.ERR_INVALID_ARG
    assert lib.orbx_bundle_adjust_prior(None, K.ctypes.data, 2, None, 1, None, 1, None, None, None, None, None, 0, 1.0,
                                        10, None) == bad
    assert lib.orbx_bundle_adjust_prior_batch(None, K.ctypes.data, 1, None, None, None, None, None, None, None, None,
                                              None, None, 0, 1.0, 10, None) == bad
    assert lib.orbx_landmarks_priors_carried_device(None, 1.0, None) == bad
    assert lib.orbx_landmarks_priors_results_device(None, None) == bad
    assert lib.orbx_landmarks_priors_fetch(None, 0, 1, None, None, None, 0, None) == bad
    assert lib.orbx_bundle_adjust_landmarks_prior_device(None, 1.0, 10, 0, None) == bad
