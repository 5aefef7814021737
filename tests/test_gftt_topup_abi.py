"""CPU check of the top-up boundary: the five entries are declared in include/orbx.h with the
reference lines they answer, exported by liborbx.so and listed in the binding's EXPORTS, and the binding offers its
method group and the view's layout."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("orbx_good_features_topup_device", "orbx_good_features_topup_results_device",
           "orbx_good_features_topup_fetch", "orbx_good_features_topup", "orbx_good_features_to_track_masked")
CITES = ("src/with_bundle_adjustment.cpp:586-593", "src/feature_tracking.cpp:68-71")


def header():
    return open(os.path.join(ROOT, "include", "orbx.h")).read()


def test_the_five_entries_are_declared_exported_and_bound(pkg):
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    lib = pkg.orbx.load()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(lib, name), name
        assert name in pkg.orbx.EXPORTS, name
    assert re.search(r"#define\s+ORBX_GFTT_TOPUP_MAX_MIN_DISTANCE\s+64\.0\b", code)
    assert re.search(r"}\s*orbx_good_features_topup_view\s*;", code)


def test_the_declarations_cite_the_reference():
    src = header()
    section = src[src.index("rank 12"):]
    for cite in CITES:
        assert cite in section, cite
    # the comment in front of each declaration names at least one of the two reference places
    for name in SYMBOLS:
        at = section.index("int %s(" % name)
        comment = section[:at].rsplit("/*", 1)[1]
        assert any(cite in comment for cite in CITES), name
    at = section.index("} orbx_good_features_topup_view;")
    assert any(cite in section[:at].rsplit("/* Device-side view", 1)[1] for cite in CITES)


def test_the_binding_offers_the_method_group(pkg):
    for m in ("good_features_topup", "good_features_topup_view", "good_features_topup_fetch",
              "good_features_topup_one", "good_features_to_track_masked"):
        assert callable(getattr(pkg.Context, m)), m
    v = pkg.orbx.GoodFeaturesTopupView
    assert C.sizeof(v) == 4 * 8 + 2 * 4
    assert [getattr(v, f).offset for f in ("counts", "carried", "points_xy", "origin", "slot_capacity", "n")] == \
        [0, 8, 16, 24, 32, 36]
