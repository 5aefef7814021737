"""CPU check of the forward-backward boundary: the four entries are declared in include/orbx.h
with the signatures the binding calls them with and the reference lines they answer, exported by liborbx.so and listed
in the binding's EXPORTS, and the binding offers its methods and the view's layout."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("orbx_lk_track_windows_fb_device", "orbx_lk_windows_fb_results_device", "orbx_lk_windows_fb_fetch",
           "orbx_lk_track_window_fb")
CITES = ("src/with_bundle_adjustment.cpp:464-499", "src/feature_tracking.cpp:166-193")


def header():
    return open(os.path.join(ROOT, "include", "orbx.h")).read()


def code():
    return re.sub(r"/\*.*?\*/", "", header(), flags=re.S)


def params(name):
    """the parameter list of a declaration as 'type name' strings"""
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code(), flags=re.S)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_the_four_entries_are_declared_exported_and_bound(pkg):
    lib = pkg.orbx.load()
    for name in SYMBOLS:
        assert params(name)[0] == "orbx_ctx* ctx", name
        assert hasattr(lib, name), name
        assert name in pkg.orbx.EXPORTS, name
    assert re.search(r"}\s*orbx_lk_windows_fb_view\s*;", code())


def test_the_signatures_are_the_plain_entries_with_the_threshold():
    plain, fb = params("orbx_lk_track_windows_device"), params("orbx_lk_track_windows_fb_device")
    assert fb == plain[:-1] + ["float fb_threshold", "void* stream"] and plain[-1] == "void* stream"
    plain, fb = params("orbx_lk_track_window"), params("orbx_lk_track_window_fb")
    assert fb == plain + ["float fb_threshold", "float* fb_d2", "int32_t* lost"]
    assert params("orbx_lk_windows_fb_results_device") == ["orbx_ctx* ctx", "orbx_lk_windows_fb_view* view"]
    assert params("orbx_lk_windows_fb_fetch") == ["orbx_ctx* ctx", "int first", "int n", "float* fb_d2",
                                                  "int32_t* lost"]


def test_the_declarations_cite_the_reference():
    src = header()
    section = src[src.index("rank 13"):]
    for cite in CITES:
        assert cite in section, cite
    for name in SYMBOLS:
        at = section.index("int %s(" % name)
        comment = section[:at].rsplit("/*", 1)[1] if name != SYMBOLS[0] else section[:at]
        assert any(cite in comment for cite in CITES), name


def test_the_binding_offers_the_methods(pkg):
    for m in ("lk_windows_fb_view", "lk_windows_fb_fetch"):
        assert callable(getattr(pkg.Context, m)), m
    for m in ("lk_track_windows", "lk_track_window"):
        p = inspect.signature(getattr(pkg.Context, m)).parameters
        assert "fb_threshold" in p and p["fb_threshold"].default is None, m
    v = pkg.orbx.LkWindowsFbView
    assert C.sizeof(v) == 2 * 8 + 3 * 4 + 4
    assert [getattr(v, f).offset for f in ("fb_d2", "lost", "slot_capacity", "window_len", "n_windows")] == \
        [0, 8, 16, 20, 24]
