"""CPU-only checks of the ctypes binding against include/orbx.h: the one prototype table (orbx.PROTOTYPES) declares
every function with the header's parameter classes, the *View structures have the header's fields, prototypes are
assigned in load() and nowhere else, and the module-level helpers that marshal device arguments refuse what the
Context methods refuse -- with the same texts, and without a GPU."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCALARS = {"int": C.c_int, "int32_t": C.c_int, "size_t": C.c_size_t, "double": C.c_double, "float": C.c_float,
           "uint64_t": C.c_uint64}
RETURNS = {"int": C.c_int, "const char*": C.c_char_p, "void": None}


def header():
    src = open(os.path.join(ROOT, "include", "orbx.h")).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def declarations():
    """{name: (return type, [parameter text, ...])} of every orbx_* function the header declares"""
    src = header()
    out = {}
    for ret, name, params in re.findall(r"^([A-Za-z_][\w \t\*]*?)\s*\b(orbx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        params = [" ".join(p.split()) for p in params.split(",")]
        out[name] = (re.sub(r"\s*\*", "*", " ".join(ret.split())), [] if params == ["void"] else params)
    assert sorted(out) == sorted(set(re.findall(r"\b(orbx_[a-z0-9_]+)\s*\(", src)))  # no declaration slipped through
    return out


def is_pointer(ctype):
    return ctype in (C.c_void_p, C.c_char_p) or (inspect.isclass(ctype) and issubclass(ctype, C._Pointer))


def test_table_against_header(pkg):
    table, decls = pkg.orbx.PROTOTYPES, declarations()
    assert len(decls) == 94 and sorted(decls) == sorted(table) and pkg.orbx.EXPORTS == list(table)
    for name, (ret, params) in decls.items():
        restype, argtypes = table[name]
        assert ret in RETURNS, "%s: return type %r is outside the header's vocabulary" % (name, ret)
        assert restype is RETURNS[ret], name
        assert len(argtypes) == len(params), name
        for i, (p, got) in enumerate(zip(params, argtypes)):
            if "*" in p:
                assert is_pointer(got), (name, i, p)
                continue
            ctype = " ".join(w for w in p.split()[:-1] if w != "const")  # (the last word is the parameter's name)
            assert ctype in SCALARS, "%s, parameter %d: type %r is outside the header's vocabulary" % (name, i, p)
            assert got is SCALARS[ctype], (name, i, p)


def test_views_against_header(pkg):
    views = re.findall(r"typedef\s+struct\s*\{([^}]*)\}\s*orbx_(\w+)_view\s*;", header())
    assert len(views) == 7
    for body, name in views:
        struct = getattr(pkg.orbx, "".join(w.capitalize() for w in name.split("_")) + "View")
        want = []
        for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
            pointer = "*" in decl
            ctype = " ".join(w for w in decl.split(",")[0].split()[:-1] if w != "const")
            assert pointer or ctype == "int32_t", "%s: field %r is neither a pointer nor int32_t" % (name, decl)
            want += [(field.replace("*", " ").split()[-1], pointer) for field in decl.split(",")]
        got = [(f, is_pointer(t)) for f, t in struct._fields_]
        assert got == want, name
        assert all(t is C.c_int32 for _, t in struct._fields_ if not is_pointer(t)), name


def test_prototypes_are_set_in_load_and_nowhere_else(pkg):
    o = pkg.orbx
    lib = o.load()
    for name, (restype, argtypes) in o.PROTOTYPES.items():
        f = getattr(lib, name)
        assert f.argtypes is not None and list(f.argtypes) == list(argtypes), name
        assert f.restype is restype, name
    src, applied = inspect.getsource(o), inspect.getsource(o.load)
    for pattern in (r"\.argtypes\s*=", r"\.restype\s*="):
        assert len(re.findall(pattern, src)) == len(re.findall(pattern, applied)) == 1, pattern
    assert "argtypes" not in src.replace(applied, "")


# ---- the helpers refuse what the methods refused ------------------------------------------------------------------
FRAMES = "frames must be (n, h, w) uint8 on the device with unit pixel stride"


def on_device(t):
    """`t` as a tensor that says it is on the device: the helpers' other checks then run without a GPU (nothing
    below reaches the library)"""
    import torch

    class OnDevice(torch.Tensor):
        is_cuda = True

    return t.as_subclass(OnDevice)


def refused(call, *args):
    with pytest.raises(ValueError) as e:
        call(*args)
    return str(e.value)


def test_frames_helper(pkg):
    import torch

    o = pkg.orbx
    batch = torch.zeros((2, 8, 16), dtype=torch.uint8)
    assert refused(o._frames_arg, batch) == FRAMES  # a CPU tensor
    assert refused(o._frames_arg, on_device(batch.float())) == FRAMES
    assert refused(o._frames_arg, on_device(batch[0])) == FRAMES  # 2-D
    assert refused(o._frames_arg, on_device(batch[:, :, ::2])) == FRAMES  # pixel stride 2
    t, n, h, w, rs, fs, uploaded = o._frames_arg(on_device(batch[:, 1:, :12]))  # and what it accepts
    assert (n, h, w, rs, fs, uploaded) == (2, 7, 12, 16, 128, False) and t.data_ptr() == batch.data_ptr() + 16


def test_stride_rule(pkg):
    import torch

    rule = pkg.orbx._frame_strides
    batch = torch.zeros((3, 8, 16), dtype=torch.uint8)
    assert rule(batch.shape, batch.stride()) == (16, 128)
    view = batch[:, 2:7, 3:12]  # a region of every frame
    assert rule(view.shape, view.stride()) == (16, 128)
    one = batch[1].expand(2, 8, 16)[:1]  # one frame taken from a batch: stride(0) == 0 after expand
    assert one.stride(0) == 0 and rule(one.shape, one.stride()) == (16, 16 * 7 + 16)
    one = batch[1:2, :5, :9]  # one frame that kept the batch's stride: never below the frame's own extent
    assert rule(one.shape, one.stride()) == (16, 128)
    assert rule((1, 8, 16), (100, 16, 1)) == (16, 16 * 7 + 16)  # a frame stride shorter than the frame
    assert rule((2, 8, 16), (100, 16, 1)) == (16, 100)  # with n > 1 the frame stride is the caller's: the entry checks it


def test_device_argument_helpers(pkg):
    import torch

    o = pkg.orbx
    # a raw address without its sizes
    assert refused(o._lk_points_arg, 0x1000, 3, None, []) == "a raw points address needs slot_capacity"
    for sizes in ((None, None, None), (3, 5, None), (None, 5, 4)):
        assert refused(o._tracks_args, 0x1000, 0x2000, *sizes) == \
            "a raw tracks address needs n_windows, slot_capacity and window_len"
    assert o._tracks_args(0x1000, 0x2000, 3, 5, 4) == (0x1000, 0x2000, 3, 5, 4, [])
    assert o._lk_points_arg(0x1000, 3, 5, []) == (0x1000, 5, False)
    # sizes that differ from the tensor's
    points = on_device(torch.zeros((3, 5, 2)))
    assert refused(o._lk_points_arg, points, 3, 6, []) == "slot_capacity differs from points.shape[1]"
    keep = []
    assert o._lk_points_arg(points, 3, None, keep) == (points.data_ptr(), 5, False) and keep[0] is points
    assert o._lk_points_arg(points, 3, 5, []) == (points.data_ptr(), 5, False)
    assert refused(o._lk_points_arg, points, 4, None, []) == \
        "points must be (n_windows, slot_capacity, 2) float32, contiguous, on the device"
    tracks, seen = on_device(torch.zeros((3, 5, 4, 2))), on_device(torch.zeros((3, 5), dtype=torch.int32))
    for sizes in ((3, 5, 5), (3, 5, None), (2, 5, 4)):
        assert refused(o._tracks_args, tracks, seen, *sizes) == \
            "n_windows / slot_capacity / window_len differ from tracks.shape"
    for sizes in ((None, None, None), (3, 5, 4)):
        got = o._tracks_args(tracks, seen, *sizes)
        assert got[:5] == (tracks.data_ptr(), seen.data_ptr(), 3, 5, 4) and got[5][0] is tracks and got[5][1] is seen
    assert refused(o._tracks_args, torch.zeros((3, 5, 4, 2)), seen, None, None, None) == \
        "tracks must be (n_windows, slots, window_len, 2) float32, contiguous, on the device"  # a CPU tensor
    assert refused(o._tracks_args, tracks, on_device(torch.zeros((3, 4), dtype=torch.int32)), None, None, None) == \
        "seen must be (n_windows, slots) int32, contiguous, on the device"
    # an LkWindowsView brings seen and the three sizes
    v = o.LkWindowsView(tracks_xy=0x1000, seen=0x2000, err=0x3000, slot_capacity=5, window_len=4, n_windows=3)
    assert o._tracks_args(v, None, None, None, None) == (0x1000, 0x2000, 3, 5, 4, [])


def test_small_helpers(pkg):
    o = pkg.orbx
    assert o._stream(None) is None and o._stream(0) is None and o._stream(0x7F00) == 0x7F00
    assert o._count(None, 2, 7) == 5 and o._count(3, 2, 7) == 3 and o._count(None, 2, lambda: 7) == 5
    assert o._count(0, 2, lambda: 1 / 0) == 0  # a given n asks nothing
    K = o._f64([[1, 0, 2], [0, 1, 3], [0, 0, 1]], (3, 3))
    assert K.dtype == "float64" and K.shape == (3, 3) and K.flags["C_CONTIGUOUS"]
    assert o._ptr(K).value == K.ctypes.data
    # float64 and int32 arrays go as typed pointers: the table's c_void_p takes them, and so does a caller's
    # POINTER(c_double) / POINTER(c_int32) prototype on the same function object
    idx = o._i32([3, 1, 2])
    for arg, typed in ((o._dp(K), C.POINTER(C.c_double)), (o._ip(idx), C.POINTER(C.c_int32))):
        assert typed.from_param(arg) is arg and C.c_void_p.from_param(arg) is not None
    assert C.cast(o._dp(K), C.c_void_p).value == K.ctypes.data and o._ip(idx)[1] == 1
